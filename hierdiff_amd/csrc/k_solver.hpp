// Second-order multistep sampling (hd_set_path_multistep / hd_multistep_step, and the stochastic hd_set_path_multistep_sde /
// hd_multistep_sde_step; no reference counterpart).  Included through kernels.hpp.
//   k_multistep_step   the third form of the posterior step: DPM-Solver++(2M) in data-prediction form, folded onto the eta = 0 row
//       x^_k = p z_t - q eps,    z_s = (a z_t - b eps) + c2 (x^_k - x^_{k-1}),    row {a, b, c2, p, q}
//   with the x part of eps mean-removed and the x part of z_s re-centred as in k_post_step (k_sampling.hpp).
// One workgroup (256 threads) per molecule, a strided loop over mol * D elements, block_sum4 for the three means: the sums of a
// molecule run in k_post_step's order, so a row with c2 == 0 gives the bits of k_post_step<1> with c == 0.  Every thread reads and
// then overwrites its own elements of the history only: x_prev and x_out may be one buffer.  Draws nothing; exact fp32.
//   k_multistep_sde_step   the fourth form: SDE-DPM-Solver++(2M), the same correction on the ancestral (eta = 1) linear row
//       x^_k = p z_t - q eps,    z_s = ((a z_t - b eps) + c xi) + c2 (x^_k - x^_{k-1}),    row {a, b, c, c2, p, q}
//   k_post_step<1>'s two passes (masked normals kept in LDS, the sums in its order) with k_multistep_step's history read / write:
//   a row with c2 == 0 gives the bits of k_post_step<1> on {a, b, c, 0} with the same draws.  Exact fp32, no atomics.
#pragma once
#include "k_sampling.hpp"

struct SolverArgs {
    const float* zt;      // [B][N][D]
    const float* eps;     // [B][N][D]
    const float* coef;    // device [rows][5], indexed by *step_ptr; null: `row`
    float row[5];         // {a, b, c2, p, q} by value (hd_multistep_step)
    const uint8_t* nm;    // [B*N] node mask bytes
    const float* x_prev;  // [B][N][D] x^_{k-1}; read only where the row's c2 != 0
    float* x_out;         // [B][N][D] x^_k (masked entries 0); may be x_prev
    float* zs;            // [B][N][D]; may be zt
    const int* step_ptr;  // device-side path position (graph replay)
    int B, N, D, mol;     // rows >= mol of a molecule (pocket rows) are left alone
};

__global__ __launch_bounds__(256) void k_multistep_step(SolverArgs a) {
    extern __shared__ float ms_s[];                // [mol * D] the un-centred z_s
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    float cf[5];
    if (a.coef) {
        const float* r = a.coef + (size_t)(a.step_ptr ? *a.step_ptr : 0) * 5;
#pragma unroll
        for (int k = 0; k < 5; ++k) cf[k] = r[k];
    } else {
#pragma unroll
        for (int k = 0; k < 5; ++k) cf[k] = a.row[k];
    }
    const bool second = cf[2] != 0.f;              // uniform over the workgroup
    const int mol = a.mol, D = a.D, total = mol * D;
    // pass 1: masked sums of eps_x per component, node count
    float se[3] = {0.f, 0.f, 0.f}, cnt = 0.f;
    for (int e = tid; e < total; e += 256) {
        const int nn = e / D, c = e - nn * D;
        if (c < 3) {
            const float ev = a.eps[((size_t)b * a.N + nn) * D + c];
#pragma unroll
            for (int k = 0; k < 3; ++k) { if (c == k) se[k] += ev; }
            if (c == 0) cnt += a.nm[b * a.N + nn] ? 1.f : 0.f;
        }
    }
    float em[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) em[k] = block_sum4(se[k], red, tid);
    cnt = block_sum4(cnt, red, tid);
#pragma unroll
    for (int k = 0; k < 3; ++k) em[k] /= cnt;
    // pass 2: x^_k out, z_s before the final re-centring (kept in LDS); its x sums
    float sv[3] = {0.f, 0.f, 0.f};
    for (int e = tid; e < total; e += 256) {
        const int nn = e / D, c = e - nn * D;
        const size_t g = ((size_t)b * a.N + nn) * D + c;
        const bool valid = a.nm[b * a.N + nn] != 0;
        const float m = valid ? 1.f : 0.f;
        const float zt = a.zt[g];
        float ev = a.eps[g];
        if (c < 3) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { if (c == k) ev -= em[k] * m; }
        }
        float v = cf[0] * zt - cf[1] * ev;         // k_post_step<1>'s expression: with c2 == 0 this is the whole update
        const float xk = cf[3] * zt - cf[4] * ev;
        if (second) {
            const float xp = a.x_prev[g];
            if (valid) v += cf[2] * (xk - xp);
        }
        a.x_out[g] = valid ? xk : 0.f;
        ms_s[e] = v;
        if (c < 3) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { if (c == k) sv[k] += v; }
        }
    }
    float mean[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) mean[k] = block_sum4(sv[k], red, tid) / cnt;
    for (int e = tid; e < total; e += 256) {
        const int nn = e / D, c = e - nn * D;
        float v = ms_s[e];
        if (c < 3) {
            const float m = a.nm[b * a.N + nn] ? 1.f : 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) { if (c == k) v -= mean[k] * m; }
        }
        a.zs[((size_t)b * a.N + nn) * D + c] = v;
    }
}

struct SdeSolverArgs {
    const float* zt;      // [B][N][D]
    const float* eps;     // [B][N][D]
    const float* coef;    // device [rows][6], indexed by *step_ptr; null: `row`
    float row[6];         // {a, b, c, c2, p, q} by value (hd_multistep_sde_step)
    const uint8_t* nm;    // [B*N] node mask bytes
    const float* x_prev;  // [B][N][D] x^_{k-1}; read only where the row's c2 != 0
    float* x_out;         // [B][N][D] x^_k (masked entries 0); may be x_prev
    float* zs;            // [B][N][D]; may be zt
    NoiseSrc noise;
    const uint32_t* draw_ptr;             // device words (graph replay), as in StepArgs
    const int* step_ptr;
    const unsigned long long* base_ptr;
    int raw_step0;
    int B, N, D, F, mol;  // rows >= mol of a molecule (pocket rows) are left alone
};

__global__ __launch_bounds__(256) void k_multistep_sde_step(SdeSolverArgs a) {
    extern __shared__ float sde_s[];               // [mol * D] masked raw normals, later the un-centred z_s
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    NoiseSrc ns = a.noise;
    if (a.base_ptr) ns.sample_base = *a.base_ptr;
    if (a.draw_ptr) {
        ns.draw = *a.draw_ptr;
        if (ns.raw_x) {
            const size_t k = (size_t)(uint32_t)(*a.step_ptr - a.raw_step0) * ns.rows * a.mol;
            ns.raw_x += k * 3;
            ns.raw_h += k * a.F;
        }
    }
    float cf[6];
    if (a.coef) {
        const float* r = a.coef + (size_t)(a.step_ptr ? *a.step_ptr : 0) * 6;
#pragma unroll
        for (int k = 0; k < 6; ++k) cf[k] = r[k];
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) cf[k] = a.row[k];
    }
    const bool noisy = cf[2] != 0.f;               // uniform over the workgroup
    const bool second = cf[3] != 0.f;
    const int mol = a.mol, D = a.D, total = mol * D;
    // pass 1: raw normals (masked) into LDS; masked sums of eps_x and of the x-noise per component, node count
    float se[3] = {0.f, 0.f, 0.f}, sn[3] = {0.f, 0.f, 0.f}, cnt = 0.f;
    for (int e = tid; e < total; e += 256) {
        const int nn = e / D, c = e - nn * D;
        const float m = a.nm[b * a.N + nn] ? 1.f : 0.f;
        float z = 0.f;
        if (noisy) {
            z = raw_noise(ns, b, nn, c, mol, a.F) * m;
            sde_s[e] = z;
        }
        if (c < 3) {
            const float ev = a.eps[((size_t)b * a.N + nn) * D + c];
#pragma unroll
            for (int k = 0; k < 3; ++k) { if (c == k) { se[k] += ev; sn[k] += z; } }
            if (c == 0) cnt += m;
        }
    }
    float em[3], nmn[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { em[k] = block_sum4(se[k], red, tid); nmn[k] = noisy ? block_sum4(sn[k], red, tid) : 0.f; }
    cnt = block_sum4(cnt, red, tid);
#pragma unroll
    for (int k = 0; k < 3; ++k) { em[k] /= cnt; nmn[k] /= cnt; }
    // pass 2: x^_k out, z_s before the final re-centring (kept in LDS); its x sums
    float sv[3] = {0.f, 0.f, 0.f};
    for (int e = tid; e < total; e += 256) {
        const int nn = e / D, c = e - nn * D;
        const size_t g = ((size_t)b * a.N + nn) * D + c;
        const bool valid = a.nm[b * a.N + nn] != 0;
        const float m = valid ? 1.f : 0.f;
        const float zt = a.zt[g];
        float ev = a.eps[g];
        float z = noisy ? sde_s[e] : 0.f;
        if (c < 3) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { if (c == k) { ev -= em[k] * m; z -= nmn[k] * m; } }
        }
        // k_post_step<1>'s expression: with c2 == 0 this is the whole update
        float v = noisy ? (cf[0] * zt - cf[1] * ev) + cf[2] * z : cf[0] * zt - cf[1] * ev;
        const float xk = cf[4] * zt - cf[5] * ev;
        if (second) {
            const float xp = a.x_prev[g];
            if (valid) v += cf[3] * (xk - xp);
        }
        a.x_out[g] = valid ? xk : 0.f;
        sde_s[e] = v;
        if (c < 3) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { if (c == k) sv[k] += v; }
        }
    }
    float mean[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) mean[k] = block_sum4(sv[k], red, tid) / cnt;
    for (int e = tid; e < total; e += 256) {
        const int nn = e / D, c = e - nn * D;
        float v = sde_s[e];
        if (c < 3) {
            const float m = a.nm[b * a.N + nn] ? 1.f : 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) { if (c == k) v -= mean[k] * m; }
        }
        a.zs[((size_t)b * a.N + nn) * D + c] = v;
    }
}
