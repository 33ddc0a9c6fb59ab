// h2_warm.h — which bytes of the fp16x2 weight planes a workgroup of mlp_fused_step_h2_kernel touches at kernel entry to bring them
// into its XCD's L2 (mlp_fused_h2.inc: the weights change every optimizer step, so each launch meets eight L2s that hold none of
// them).  A plane is cut into H2_WARM_SHARES shares of whole 128-byte lines; a workgroup reads ONE dword of every line of one share
// of each plane, thread t the line t, t + threads, ... of the share.  Workgroups are dealt round-robin over the 8 XCDs, so
// (block >> 3) & 31 numbers the 32 workgroups of one XCD 0 .. 31 and together they cover the planes.  Placement is for speed only:
// any grid and any dispatch order read valid addresses, a workgroup without a tile reads its share too.
// Plain C++ (the arithmetic is compiled for the host by tests/test_fused_h2_warm_cpu.py).
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define H2_WARM_FN __host__ __device__ inline
#else
#define H2_WARM_FN inline
#endif

constexpr unsigned H2_WARM_SHARES = 32, H2_WARM_LINE = 128;

H2_WARM_FN constexpr unsigned h2_warm_share(unsigned block) { return (block >> 3) & (H2_WARM_SHARES - 1); }
// lines of a plane of `bytes` bytes, lines per share (the last share may be shorter), loads per thread
H2_WARM_FN constexpr unsigned h2_warm_lines(unsigned bytes) { return (bytes + H2_WARM_LINE - 1) / H2_WARM_LINE; }
H2_WARM_FN constexpr unsigned h2_warm_share_lines(unsigned bytes) { return (h2_warm_lines(bytes) + H2_WARM_SHARES - 1) / H2_WARM_SHARES; }
H2_WARM_FN constexpr unsigned h2_warm_loads(unsigned bytes, unsigned threads) { return (h2_warm_share_lines(bytes) + threads - 1) / threads; }
// byte offset of the dword that thread `t` reads in its load `j` of share `share`: a line past the share's (or the plane's) end is
// clamped to the last line of the share (of the plane) -- the load is issued regardless, no branch around it
H2_WARM_FN constexpr unsigned h2_warm_offset(unsigned bytes, unsigned share, unsigned j, unsigned t, unsigned threads)
{
    const unsigned per = h2_warm_share_lines(bytes), lines = h2_warm_lines(bytes);
    unsigned first = share * per, end = first + per;
    if (end > lines) end = lines;
    if (first >= end) first = end - 1;              // (an empty last share: re-read the plane's last line)
    unsigned line = first + j * threads + t;
    if (line >= end) line = end - 1;
    unsigned off = line * H2_WARM_LINE;
    if (off + 4 > bytes) off = (bytes - 4) & ~3u;   // (a plane that ends inside its last line)
    return off;
}
