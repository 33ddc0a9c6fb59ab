// fly_render.hip — the recording renderer (fly_render, include/flyhip.h): one chase-camera view of a recorded pose per
// frame, ray cast against the fly's ~23 analytic primitives and the ground plane.
//
// Shape: one thread per pixel, one 256-thread workgroup per 64 x 4 pixel tile, frames on grid z.  A wave owns one 64-pixel
// row segment, so its RGBA8 dword stores are one contiguous 256-byte run (a 16 x 16 tile would split them into four
// 64-byte runs).  Wave 0 first builds the frame's scene -- camera basis and every primitive in camera-relative world
// coordinates -- in LDS, once per workgroup; then every thread casts its primary ray and, where the light can reach the
// surface, one shadow ray.  Camera-relative coordinates keep fp32 exact enough far from the origin (a fly at x = 1000 mm).
// tests/render_ref.py is the float64 statement of the same scene.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flyhip.h"
#include "launch.h"

namespace {

constexpr int RT_W = 64, RT_H = 4, RT_THREADS = RT_W * RT_H;
constexpr int NSPH = 1 + FLY_NUM_ABDOMEN;                        // head, then the abdomen points
constexpr int NCAP = 2 * FLY_NUM_LEGS + FLY_NUM_ABDOMEN - 1;     // femur, tibia of every leg, then the abdomen links

struct V3 {
    float x, y, z;
};
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 normalize(V3 a) { return a * (1.0f / sqrtf(dot(a, a))); }
__device__ __forceinline__ V3 xyz(float4 v) { return {v.x, v.y, v.z}; }

struct Scene {
    float cam[3];                 // camera position (world)
    V3 fw, rt, up;                // camera basis
    V3 ec;                        // thorax centre, camera-relative
    float eR[9];                  // body -> world rotation, row major
    V3 einv;                      // 1 / thorax semi-axes
    float4 sph[NSPH];             // centre (camera-relative), radius
    float4 capa[NCAP];            // end a (camera-relative), radius
    float4 capb[NCAP];            // end b (camera-relative), class id
};

__device__ __forceinline__ V3 rot(const float* R, V3 v)
{
    return {R[0] * v.x + R[1] * v.y + R[2] * v.z, R[3] * v.x + R[4] * v.y + R[5] * v.z, R[6] * v.x + R[7] * v.y + R[8] * v.z};
}
__device__ __forceinline__ V3 rot_t(const float* R, V3 v)
{
    return {R[0] * v.x + R[3] * v.y + R[6] * v.z, R[1] * v.x + R[4] * v.y + R[7] * v.z, R[2] * v.x + R[5] * v.y + R[8] * v.z};
}

// wave 0: lane l < 6 builds leg l's two capsules, lane l < 5 abdomen sphere l (and link l -> l + 1 for l < 4), lane 0 the
// camera, the thorax and the head
__device__ void build_scene(Scene& S, const FlyConfig* __restrict__ c, const float* __restrict__ pose, const FlyRenderConfig& rc,
                            int lane)
{
    const V3 pos = {pose[0], pose[1], pose[2]};
    const float qx = pose[3], qy = pose[4], qz = pose[5], qw = pose[6];
    float R[9];
    R[0] = 1.0f - 2.0f * (qy * qy + qz * qz); R[1] = 2.0f * (qx * qy - qz * qw); R[2] = 2.0f * (qx * qz + qy * qw);
    R[3] = 2.0f * (qx * qy + qz * qw); R[4] = 1.0f - 2.0f * (qx * qx + qz * qz); R[5] = 2.0f * (qy * qz - qx * qw);
    R[6] = 2.0f * (qx * qz - qy * qw); R[7] = 2.0f * (qy * qz + qx * qw); R[8] = 1.0f - 2.0f * (qx * qx + qy * qy);
    const V3 cam = {pos.x + rc.cam_offset[0], pos.y + rc.cam_offset[1], rc.cam_offset[2]};
    const V3 rel = pos - cam;                                        // root, camera-relative
    if (lane < FLY_NUM_LEGS) {
        const int l = lane;
        const float* q = pose + 7 + 3 * l;
        const float* p0 = c->dof_pose + 3 * l;
        const float psi = c->leg_azimuth[l] + c->leg_sigma[l] * (q[0] - p0[0]);
        const float al = c->alpha0 + (q[1] - p0[1]);
        const float gm = al + c->beta0 + (q[2] - p0[2]);
        const float Lf = c->femur_len, Lt = c->tibia_len;
        const float cp = cosf(psi), sp = sinf(psi), ca = cosf(al), sa = sinf(al);
        const float rho = Lf * ca + Lt * cosf(gm), zeta = Lf * sa + Lt * sinf(gm);
        const V3 att = {c->leg_attach[l][0], c->leg_attach[l][1], c->leg_attach[l][2]};
        const V3 knee = att + V3{cp * Lf * ca, sp * Lf * ca, Lf * sa};
        const V3 tip = att + V3{cp * rho, sp * rho, zeta};
        const V3 wa = rel + rot(R, att), wk = rel + rot(R, knee), wt = rel + rot(R, tip);
        const float cls = (float)(FLY_RID_LEG0 + l);
        S.capa[2 * l] = make_float4(wa.x, wa.y, wa.z, FLY_R_LEG_RADIUS);
        S.capb[2 * l] = make_float4(wk.x, wk.y, wk.z, cls);
        S.capa[2 * l + 1] = make_float4(wk.x, wk.y, wk.z, FLY_R_LEG_RADIUS);
        S.capb[2 * l + 1] = make_float4(wt.x, wt.y, wt.z, cls);
    }
    if (lane < FLY_NUM_ABDOMEN) {
        const int k = lane;
        const V3 a = rel + rot(R, V3{c->abdomen_pts[k][0], c->abdomen_pts[k][1], c->abdomen_pts[k][2]});
        S.sph[1 + k] = make_float4(a.x, a.y, a.z, FLY_R_ABDOMEN_SPHERE);
        if (k + 1 < FLY_NUM_ABDOMEN) {
            const V3 b = rel + rot(R, V3{c->abdomen_pts[k + 1][0], c->abdomen_pts[k + 1][1], c->abdomen_pts[k + 1][2]});
            S.capa[2 * FLY_NUM_LEGS + k] = make_float4(a.x, a.y, a.z, FLY_R_ABDOMEN_LINK);
            S.capb[2 * FLY_NUM_LEGS + k] = make_float4(b.x, b.y, b.z, (float)FLY_RID_ABDOMEN);
        }
    }
    if (lane == 0) {
        S.cam[0] = cam.x; S.cam[1] = cam.y; S.cam[2] = cam.z;
        const V3 fw = normalize(V3{-rc.cam_offset[0], -rc.cam_offset[1], rc.look_z - rc.cam_offset[2]});
        const V3 rt = normalize(cross(fw, V3{0.0f, 0.0f, 1.0f}));
        S.fw = fw; S.rt = rt; S.up = cross(rt, fw);
        S.ec = rel;
        for (int i = 0; i < 9; ++i) S.eR[i] = R[i];
        const float axes[3] = {FLY_R_THORAX_AXES};
        S.einv = {1.0f / axes[0], 1.0f / axes[1], 1.0f / axes[2]};
        const float hc[3] = {FLY_R_HEAD_CENTER};
        const V3 h = rel + rot(R, V3{hc[0], hc[1], hc[2]});
        S.sph[0] = make_float4(h.x, h.y, h.z, FLY_R_HEAD_RADIUS);
    }
}

// nearest intersection in front of o (t > 0), or -1; d is unit length.  A ray that starts inside a primitive misses it:
// primary rays start at the camera, shadow rays on a visible surface, and neither is inside a primitive.
__device__ __forceinline__ float hit_sphere(V3 o, V3 d, float4 s)
{
    const V3 oc = o - xyz(s);
    const float b = dot(oc, d), cc = dot(oc, oc) - s.w * s.w;
    const float h = b * b - cc;
    return h < 0.0f ? -1.0f : -b - sqrtf(h);
}

__device__ __forceinline__ float hit_capsule(V3 o, V3 d, float4 A, float4 B)
{
    const V3 a = xyz(A), b = xyz(B);
    const float r = A.w;
    const V3 ba = b - a, oa = o - a;
    const float baba = dot(ba, ba), bard = dot(ba, d), baoa = dot(ba, oa), rdoa = dot(d, oa), oaoa = dot(oa, oa);
    const float qa = baba - bard * bard, qb = baba * rdoa - baoa * bard, qc = baba * oaoa - baoa * baoa - r * r * baba;
    float h = qb * qb - qa * qc;
    if (h < 0.0f) return -1.0f;
    const float t = (-qb - sqrtf(h)) / qa;
    const float y = baoa + t * bard;
    if (y > 0.0f && y < baba) return t;                              // the cylinder
    const V3 oc = y <= 0.0f ? oa : o - b;                             // an end cap
    const float cb = dot(d, oc), cc = dot(oc, oc) - r * r;
    h = cb * cb - cc;
    return h > 0.0f ? -cb - sqrtf(h) : -1.0f;
}

__device__ __forceinline__ float hit_ellipsoid(const Scene& S, V3 o, V3 d)
{
    const V3 ob = rot_t(S.eR, o - S.ec), db = rot_t(S.eR, d);
    const V3 os = {ob.x * S.einv.x, ob.y * S.einv.y, ob.z * S.einv.z}, ds = {db.x * S.einv.x, db.y * S.einv.y, db.z * S.einv.z};
    const float a = dot(ds, ds), b = dot(os, ds), cc = dot(os, os) - 1.0f;
    const float h = b * b - a * cc;
    return h < 0.0f ? -1.0f : (-b - sqrtf(h)) / a;
}

__device__ __forceinline__ bool occluded(const Scene& S, V3 o, V3 d)
{
    if (hit_ellipsoid(S, o, d) > 0.0f) return true;
    for (int i = 0; i < NSPH; ++i)
        if (hit_sphere(o, d, S.sph[i]) > 0.0f) return true;
    for (int i = 0; i < NCAP; ++i)
        if (hit_capsule(o, d, S.capa[i], S.capb[i]) > 0.0f) return true;
    return false;
}

__device__ __forceinline__ uint32_t quantise(float x)
{
    return (uint32_t)floorf(fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f + 0.5f);
}

__global__ __launch_bounds__(RT_THREADS) void fly_render_kernel(const FlyConfig* __restrict__ c, const float* __restrict__ poses,
                                                                FlyRenderConfig rc, uint32_t* __restrict__ rgba_out,
                                                                uint8_t* __restrict__ id_out)
{
    __shared__ Scene S;
    const int f = blockIdx.z;
    if (threadIdx.x < 64) build_scene(S, c, poses + (long)f * FLY_POSE_FLOATS, rc, threadIdx.x);
    __syncthreads();
    const int W = rc.width, H = rc.height;
    const int px = blockIdx.x * RT_W + (threadIdx.x & (RT_W - 1)), py = blockIdx.y * RT_H + threadIdx.x / RT_W;
    if (px >= W || py >= H) return;

    const float th = tanf(0.5f * rc.fov_y_deg * 0.017453292519943295f);
    const float sx = (2.0f * ((float)px + 0.5f) / (float)W - 1.0f) * th * ((float)W / (float)H);
    const float sy = (1.0f - 2.0f * ((float)py + 0.5f) / (float)H) * th;
    const V3 d = normalize(S.fw + S.rt * sx + S.up * sy);
    const V3 o = {0.0f, 0.0f, 0.0f};

    // nearest hit: the ground first, then the primitives in a fixed order, strictly nearer wins (render_ref.py: same order)
    float best = 3.0e38f;
    int kind = 0, idx = 0, cls = FLY_RID_SKY;        // kind 0 sky, 1 ground, 2 thorax, 3 sphere, 4 capsule
    {
        const float t = -S.cam[2] / d.z;
        if (t > 0.0f && t < best) { best = t; kind = 1; cls = FLY_RID_GROUND; }
    }
    {
        const float t = hit_ellipsoid(S, o, d);
        if (t > 0.0f && t < best) { best = t; kind = 2; cls = FLY_RID_BODY; }
    }
    for (int i = 0; i < NSPH; ++i) {
        const float t = hit_sphere(o, d, S.sph[i]);
        if (t > 0.0f && t < best) { best = t; kind = 3; idx = i; cls = i == 0 ? FLY_RID_BODY : FLY_RID_ABDOMEN; }
    }
    for (int i = 0; i < NCAP; ++i) {
        const float t = hit_capsule(o, d, S.capa[i], S.capb[i]);
        if (t > 0.0f && t < best) { best = t; kind = 4; idx = i; cls = (int)S.capb[i].w; }
    }

    float rgb[3] = {FLY_R_SKY_RGB};
    if (kind != 0) {
        const V3 p = d * best;
        V3 n;
        float base[3];
        if (kind == 1) {
            n = {0.0f, 0.0f, S.cam[2] >= 0.0f ? 1.0f : -1.0f};
            const float wx = S.cam[0] + p.x, wy = S.cam[1] + p.y;
            const int parity = ((int)floorf(wx / FLY_R_CHECKER) + (int)floorf(wy / FLY_R_CHECKER)) & 1;
            const float ga[3] = {FLY_R_GROUND_RGB_A}, gb[3] = {FLY_R_GROUND_RGB_B};
            for (int k = 0; k < 3; ++k) base[k] = parity ? gb[k] : ga[k];
        } else {
            if (kind == 2) {
                const V3 pb = rot_t(S.eR, p - S.ec);
                n = normalize(rot(S.eR, V3{pb.x * S.einv.x * S.einv.x, pb.y * S.einv.y * S.einv.y, pb.z * S.einv.z * S.einv.z}));
            } else if (kind == 3) {
                n = normalize(p - xyz(S.sph[idx]));
            } else {
                const V3 a = xyz(S.capa[idx]), ba = xyz(S.capb[idx]) - a, pa = p - a;
                const float baba = dot(ba, ba);
                const float hh = baba > 0.0f ? fminf(fmaxf(dot(pa, ba) / baba, 0.0f), 1.0f) : 0.0f;
                n = normalize(pa - ba * hh);
            }
            const float cb[3] = {FLY_R_BODY_RGB}, ca[3] = {FLY_R_ABDOMEN_RGB}, cl[3] = {FLY_R_LEG_RGB};
            const float* src = cls == FLY_RID_BODY ? cb : cls == FLY_RID_ABDOMEN ? ca : cl;
            for (int k = 0; k < 3; ++k) base[k] = src[k];
        }
        const float lv[3] = {FLY_R_LIGHT};
        const V3 L = normalize(V3{lv[0], lv[1], lv[2]});
        float ndl = fmaxf(dot(n, L), 0.0f);
        if (ndl > 0.0f && occluded(S, p + n * FLY_R_SHADOW_BIAS, L)) ndl = 0.0f;
        const float shade = FLY_R_AMBIENT + (1.0f - FLY_R_AMBIENT) * ndl;
        for (int k = 0; k < 3; ++k) rgb[k] = base[k] * shade;
    }
    const long off = ((long)f * H + py) * W + px;
    rgba_out[off] = quantise(rgb[0]) | (quantise(rgb[1]) << 8) | (quantise(rgb[2]) << 16) | 0xFF000000u;
    if (id_out) id_out[off] = (uint8_t)cls;
}

}  // namespace

extern "C" hipError_t flyhip_launch_render(const FlyConfig* dcfg, const float* poses, int frames, const FlyRenderConfig* rc,
                                           uint32_t* rgba_out, uint8_t* id_out, void* stream)
{
    const dim3 grid((unsigned)((rc->width + RT_W - 1) / RT_W), (unsigned)((rc->height + RT_H - 1) / RT_H), (unsigned)frames);
    hipLaunchKernelGGL(fly_render_kernel, grid, dim3(RT_THREADS), 0, (hipStream_t)stream, dcfg, poses, *rc, rgba_out, id_out);
    return hipGetLastError();
}
