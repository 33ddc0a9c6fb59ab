// domain_rand.h — per-env physics domain randomisation (fly_set_randomization): the slot layout shared by the handle
// (flyhip_abi.hip), the registration draw (domain_rand.hip) and the DR instantiations of the env body (fly_body.inc), and the
// device helpers: the hash, the draw, and loading and storing a table row.
//
//   table  f32 [N][FLY_DR_ROW]: m[6] | draw count (int32 bits) | 0      the multipliers env e runs FlyDyn on
//
// A draw is a pure function of (seed, e, k, j) (include/flyhip.h): k = the env's count before the draw, uint32 wrapping.
#ifndef DOMAIN_RAND_H
#define DOMAIN_RAND_H

#include "flyhip.h"
#include "obs_norm.h"

// The handle's device copy of FlyConfig: the config | the obs-norm table pointer (OBS_NORM_SLOT) | this slot.  The DR kernels
// read it through the config pointer they already receive, so no launch gains an argument.
struct DrSlot {
    float* table;                 // [N][FLY_DR_ROW], 16-byte aligned
    FlyRandomization r;           // ranges and seed
};
constexpr unsigned long DR_SLOT = OBS_NORM_SLOT + 16;
constexpr unsigned long DR_CONFIG_BYTES = DR_SLOT + ((sizeof(DrSlot) + 15) & ~15UL);   // what fly_create allocates
static_assert(FLY_DR_PARAMS == 6 && FLY_DR_ROW == 8, "a row is m[6] | count | 0: two 16-byte stores");

#ifdef __HIPCC__
__device__ __forceinline__ const DrSlot* dr_slot(const FlyConfig* c)
{
    return reinterpret_cast<const DrSlot*>(reinterpret_cast<const char*>(c) + DR_SLOT);
}

__device__ __forceinline__ uint32_t dr_lowbias32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// the six multipliers of env e's draw number k (every lane of the env computes the same bits)
__device__ __forceinline__ void dr_draw(const FlyConfig* c, uint32_t e, uint32_t k, float m[FLY_DR_PARAMS])
{
    const DrSlot* s = dr_slot(c);
    const uint32_t key = dr_lowbias32(s->r.seed ^ dr_lowbias32(e));
    const uint32_t ctr = dr_lowbias32(key + k);
#pragma unroll
    for (int j = 0; j < FLY_DR_PARAMS; ++j) {
        const uint32_t h = dr_lowbias32(ctr + 0x9E3779B9u * (uint32_t)(j + 1));
        const float u = __fmul_rn((float)(h >> 8), 5.9604644775390625e-8f);          // exact: 0 <= u < 1
        const float lo = s->r.lo[j], hi = s->r.hi[j];
        m[j] = __fadd_rn(lo, __fmul_rn(__fsub_rn(hi, lo), u));
    }
}

__device__ __forceinline__ void dr_load_row(const FlyConfig* c, long e, float m[FLY_DR_PARAMS], uint32_t& k)
{
    const float4* row = reinterpret_cast<const float4*>(dr_slot(c)->table + e * FLY_DR_ROW);
    const float4 a = row[0], b = row[1];
    m[0] = a.x; m[1] = a.y; m[2] = a.z; m[3] = a.w; m[4] = b.x; m[5] = b.y;
    k = __builtin_bit_cast(uint32_t, b.z);
}

// one lane per env stores its row: two ordinary 16-byte vector stores
__device__ __forceinline__ void dr_store_row(const FlyConfig* c, long e, const float m[FLY_DR_PARAMS], uint32_t k)
{
    float4* row = reinterpret_cast<float4*>(dr_slot(c)->table + e * FLY_DR_ROW);
    row[0] = make_float4(m[0], m[1], m[2], m[3]);
    row[1] = make_float4(m[4], m[5], __builtin_bit_cast(float, k), 0.0f);
}
#endif

#endif
