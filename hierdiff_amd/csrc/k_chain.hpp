// Recording a sampling trajectory inside the path loop (hd_set_chain / hd_chain_attach; the reference's sample_chain,
// en_diffusion.py:669-710).  Included through kernels.hpp.
//   k_chain_frame<0>   frame f = frame_of[k] of the sink <- the state z behind transition k, in data units
//   k_chain_frame<1>   the same frame <- the data prediction x^ = 1 / alpha_t (z_t - sigma_t eps^) of transition k (compute_x_pred)
// with `unnormalize` applied: x = v nv0, h = (v nv1 + nb1) mask, padded rows exactly 0 - a multiply and then an add, never fused, so a
// frame holds the bits of the torch expression on the same state.  frame_of[k] < 0: the whole grid returns (most transitions of a long
// chain keep nothing).  The destination is read from a device word, not from the launch arguments: a captured transition records
// into whatever tensor the loop's state kernel put there.  One workgroup (256 threads) per molecule as k_guide_combine, a strided
// loop over its N * D elements, no LDS: any N * D.  Draws nothing.
#pragma once
#include "common.hpp"

struct ChainArgs {
    const float* z;        // [B][N][D] the state (WHAT 0) / z_t (WHAT 1)
    const float* eps;      // [B][N][D] network output (WHAT 1)
    const uint8_t* nm;     // [B*N] node mask bytes
    const int* frame_of;   // [K] frame of every path position, -1: none
    const float* alsig;    // [K][2] {alpha_t, sigma_t} of every transition's departure level (WHAT 1)
    float* const* dst_w;   // device word holding the sink [frames][B][N][D] (graph replay); null: `dst`
    float* dst;
    const int* step_ptr;   // device-side path position (graph replay); null: `k`
    int k;
    float nv0, nv1, nb1;   // norm_values[0], norm_values[1], norm_biases[1]
    int B, N, D;
};

template <int WHAT>
__global__ __launch_bounds__(256) void k_chain_frame(ChainArgs a) {
    const int k = a.step_ptr ? *a.step_ptr : a.k;
    const int f = a.frame_of[k];
    if (f < 0) return;                             // uniform over the grid
    const int tid = threadIdx.x, b = blockIdx.x;
    const int D = a.D, total = a.N * D;
    const size_t base = (size_t)b * total;
    float* out = (a.dst_w ? *a.dst_w : a.dst) + (size_t)f * a.B * total + base;
    const uint8_t* nm = a.nm + (size_t)b * a.N;
    float ra = 1.f, sg = 0.f;
    if constexpr (WHAT == 1) { ra = __fdiv_rn(1.f, a.alsig[2 * k]); sg = a.alsig[2 * k + 1]; }
    for (int e = tid; e < total; e += 256) {
        const int nn = e / D, c = e - nn * D;
        float v = a.z[base + e];
        if constexpr (WHAT == 1) v = __fmul_rn(ra, __fsub_rn(v, __fmul_rn(sg, a.eps[base + e])));
        const float o = c < 3 ? __fmul_rn(v, a.nv0) : __fadd_rn(__fmul_rn(v, a.nv1), a.nb1);
        out[e] = nm[nn] ? o : 0.f;
    }
}
