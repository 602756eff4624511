// Predictor-corrector sampling (hd_set_corrector / hd_corrector_attach / hd_langevin_step; no reference counterpart).  Included through
// kernels.hpp.
//   k_langevin_step   one unadjusted Langevin step on z at a fixed noise level, on the score the network call before it defines:
//                     z' = (z - (g_b sigma_t) eps~) + (sigma_t sqrt(2 g_b)) xi~, the x part re-centred over the valid nodes
// which is z + delta score + sqrt(2 delta) xi with score = -eps^ / sigma_t and delta = g_b sigma_t^2.  eps~ is eps^ with its x part
// freed of the mean over the valid nodes, xi~ the masked normals with their x part freed of its mean, both as k_post_step forms them.
// The row is {sigma_t, q_k, g_max_k}: the gain is g_b = q_k ("fixed"), or - `adaptive` - g_b = min(g_max_k, q_k n_xi^2 / n_eps^2) with
// n_xi^2 = sum xi~^2 and n_eps^2 = sum eps~^2 over the valid nodes and all D columns (Song et al. 2021, q_k = 2 r^2 alpha^2_{t|s}).
// One workgroup (256 threads) per molecule, dynamic LDS = N * D floats: every normal is produced once and kept there, later the
// un-centred z'.  The two means and the node count are double sums (one guide_block_sum<7>), rounded once to the fp32 means the update
// subtracts as k_post_step does; the two squared norms are double sums of the deviations from the double means, strided per thread,
// then ONE guide_block_sum<2>: every order depends on (N, D) alone, and the gain is that of the fp32 inputs to about 1e-15.  The two
// coefficients are formed in double and rounded once; the last re-centring is k_post_step's fp32 one.  No atomics, nothing goes to
// global memory between the passes.
// Contracts: masked rows are never written; a row with q_k == 0 draws nothing and writes nothing (out is not touched at all); a
// molecule keeps the bits of z (gain 0 in `gain`) when it has no valid node, when n_eps^2 is not greater than 0, when a norm or the
// gain is not finite, or when g_b == 0.
#pragma once
#include "common.hpp"
#include "k_sampling.hpp"
#include "k_guide.hpp"

struct LangevinArgs {
    const float* z;         // [B][N][D]
    const float* eps;       // [B][N][D] the network output at this level (with every loop term in it)
    const uint8_t* nm;      // [B*N] node mask bytes
    float* out;             // [B][N][D]; may be z itself (every thread reads its elements before the last barrier and writes behind it)
    double* gain;           // [B] g_b, or null
    const float* rows;      // device [K][3] {sigma_t, q_k, g_max_k} (path loop); null: `row`
    float row[3];
    const int* step_ptr;    // device-side path position (graph replay); null: `k`
    int k;
    NoiseSrc noise;
    const uint32_t* draw_ptr;             // optional device-side draw word (graph replay); overrides noise.draw
    const unsigned long long* base_ptr;   // optional device-side first global sample id (graph replay); overrides noise.sample_base
    int adaptive;           // 1: "snr", 0: "fixed"
    int B, N, D, F;
};

__global__ __launch_bounds__(256) void k_langevin_step(LangevinArgs a) {
    extern __shared__ float lv_s[];                // [N * D] masked raw normals, later the un-centred z'
    __shared__ float red[4];
    __shared__ double redd[4 * 7];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int k = a.step_ptr ? *a.step_ptr : a.k;
    const float* row = a.rows ? a.rows + (size_t)k * 3 : a.row;
    const float sigma_t = row[0], q = row[1], gmax = row[2];
    if (q == 0.f) return;                          // uniform over the grid
    NoiseSrc ns = a.noise;
    if (a.base_ptr) ns.sample_base = *a.base_ptr;
    if (a.draw_ptr) ns.draw = *a.draw_ptr;
    const int N = a.N, D = a.D, total = N * D;
    const size_t base = (size_t)b * total;
    const float* zt = a.z + base;
    const float* ep = a.eps + base;
    float* out = a.out + base;
    const uint8_t* nm = a.nm + (size_t)b * N;
    // pass 1: raw normals (masked) into LDS; masked sums of eps_x and of the x-noise per component, node count
    double s7[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // sum eps_x [3], sum xi_x [3], valid nodes
    for (int e = tid; e < total; e += 256) {
        const int nn = e / D, c = e - nn * D;
        const bool valid = nm[nn] != 0;
        const float xi = valid ? raw_noise(ns, b, nn, c, N, a.F) : 0.f;
        lv_s[e] = xi;
        if (c < 3) {
            const float ev = valid ? ep[e] : 0.f;
#pragma unroll
            for (int j = 0; j < 3; ++j) { if (c == j) { s7[j] += (double)ev; s7[3 + j] += (double)xi; } }
            if (c == 0 && valid) s7[6] += 1.0;
        }
    }
    guide_block_sum<7>(s7, redd, tid);
    if (s7[6] == 0.0) {                            // no valid node: nothing to write (uniform over the workgroup)
        if (a.gain && tid == 0) a.gain[b] = 0.0;
        return;
    }
    const float cnt = (float)s7[6];
    double emd[3], nmd[3];
    float em[3], nmn[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { emd[j] = s7[j] / s7[6]; nmd[j] = s7[3 + j] / s7[6]; em[j] = (float)emd[j]; nmn[j] = (float)nmd[j]; }
    // pass 2: the two squared norms over the valid nodes and all D columns, in double
    double nrm[2] = {0.0, 0.0};                    // n_xi^2, n_eps^2
    for (int e = tid; e < total; e += 256) {
        const int nn = e / D, c = e - nn * D;
        if (!nm[nn]) continue;
        double ev = (double)ep[e], xi = (double)lv_s[e];
        if (c < 3) {
#pragma unroll
            for (int j = 0; j < 3; ++j) { if (c == j) { ev -= emd[j]; xi -= nmd[j]; } }
        }
        nrm[0] += xi * xi;
        nrm[1] += ev * ev;
    }
    guide_block_sum<2>(nrm, redd, tid);            // every thread holds the same sums: the gain needs no broadcast
    double g = 0.0;
    if (nrm[1] > 0.0 && nrm[0] - nrm[0] == 0.0 && nrm[1] - nrm[1] == 0.0) {
        g = (double)q;
        if (a.adaptive) {
            const double ga = (double)q * nrm[0] / nrm[1];
            g = ga < (double)gmax ? ga : (double)gmax;
        }
        if (!(g - g == 0.0)) g = 0.0;              // not finite
    }
    if (a.gain && tid == 0) a.gain[b] = g;
    if (g == 0.0) {                                // the molecule keeps its bits (uniform over the workgroup)
        if (out != zt)
            for (int e = tid; e < total; e += 256) { if (nm[e / D]) out[e] = zt[e]; }
        return;
    }
    const float c_eps = (float)(g * (double)sigma_t), c_xi = (float)((double)sigma_t * sqrt(2.0 * g));
    // pass 3: z' before the final re-centring into LDS, its x sums over the valid nodes
    float sv[3] = {0.f, 0.f, 0.f};
    for (int e = tid; e < total; e += 256) {
        const int nn = e / D, c = e - nn * D;
        const bool valid = nm[nn] != 0;
        float ev = valid ? ep[e] : 0.f, xi = lv_s[e];
        if (c < 3 && valid) {
#pragma unroll
            for (int j = 0; j < 3; ++j) { if (c == j) { ev -= em[j]; xi -= nmn[j]; } }
        }
        const float v = valid ? (zt[e] - c_eps * ev) + c_xi * xi : 0.f;
        lv_s[e] = v;
        if (c < 3) {
#pragma unroll
            for (int j = 0; j < 3; ++j) { if (c == j) sv[j] += v; }
        }
    }
    float mean[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) mean[j] = block_sum4(sv[j], red, tid) / cnt;
    // pass 4: re-centre and write the valid rows
    for (int e = tid; e < total; e += 256) {
        const int nn = e / D, c = e - nn * D;
        if (!nm[nn]) continue;
        float v = lv_s[e];
        if (c < 3) {
#pragma unroll
            for (int j = 0; j < 3; ++j) { if (c == j) v -= mean[j]; }
        }
        out[e] = v;
    }
}
