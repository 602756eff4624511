// Diverse sampling (hd_set_diversity / hd_diversity_attach / hd_diverse_eps / hd_diversity_energy; no reference counterpart): the rows
// of a group repel each other by their aligned RMSD.  Included through kernels.hpp.
//   k_diverse_eps      eps_x += project(clip(s_g lambda_k dPhi/dx)) with Phi evaluated on the transition's data predictions x^0
//   k_diverse_energy   Phi per group and the aligned RMSD matrix [P][P] of given data-unit positions
// The batch is G groups of P rows, group g owns rows g P .. g P + P - 1; groups never interact.  Per pair p < q of a group, in double on
// the fp32 x^0 (A = the nodes valid in both rows, n = |A|):
//   c_p, c_q = the centroids over A,  S = sum_A (x_p - c_p)(x_q - c_q)^T,  R = argmax_{SO(3)} tr(R^T S) (k_kabsch.hpp: a proper rotation,
//   mirror images stay apart),  r_i = (x_p,i - c_p) - R (x_q,i - c_q),  d2 = sum_A |r_i|^2 / n,  e = exp(-d2 / (2 l^2))
//   Phi = kappa sum_{p<q} e,   dPhi/dx_p,i = -(kappa / (l^2 n)) e r_i,   dPhi/dx_q,i = -(kappa / (l^2 n)) e ((x_q,i - c_q) - R^T (x_p,i - c_p))
// (exact without dR/dx: R maximises and sum_A r = 0).  A pair with n <= 1, or with a non-finite coordinate on a node of A, contributes
// nothing to either side.  n = 2 or collinear nodes: R is some maximiser, d2 is unique and the gradient finite.
// One workgroup (256 threads) per group.  x^0 of its P rows lies in dynamic LDS, behind it one record (q of R, c_p, c_q, e, n) per pair.
// Pair j = 4 l + w (+ 256 per round) is fitted by lane l of wave w alone - the four waves share the Jacobi solves - with three sequential
// sums over i = 0 .. N - 1; then one thread per (row, node) adds the partners q in ascending order; then one thread per (row, component)
// sums the clipped steps over i = 0 .. N - 1 for the projection.  Every order depends on (N, P) alone, never on where the group sits in the
// batch.  No atomics; the clipped steps pass through a topology-owned double buffer as in k_restrain_eps.  Draws nothing.
#pragma once
#include "common.hpp"
#include "k_kabsch.hpp"

#define DV_MAX_P 32
#define DV_REC 12           // doubles of LDS per pair: q [4], c_p [3], c_q [3], e, n (0: contributes nothing)

struct DiverseArgs {
    const float* z;         // [B][N][D] z_t
    const float* eps;       // [B][N][D] network output
    float* out;             // [B][N][D]; may be eps itself (then only the x columns of valid nodes are written)
    const uint8_t* nm;      // [B*N] node mask bytes
    const float* scale;     // [scale_rows] s_g, scale_rows = 1 (shared) or B / P
    const float* rows;      // device [K][4] {alpha_t, sigma_t, lambda_k, clip_k} (path loop); null: `row`
    float row[4];
    const int* step_ptr;    // device-side path position (graph replay); null: `k`
    int k;
    double* step;           // [B][N][3] scratch: the clipped steps before the projection
    double kappa, inv_l2;   // kappa, 1 / l^2
    float nv0;
    int scale_rows, P, B, N, D;
};

struct DiverseEnergyArgs {
    const float* x;         // [B][N][3] positions in data units
    const uint8_t* nm;
    double* phi;            // [G]
    double* rmsd;           // [G][P][P]; null: not wanted
    double kappa, inv_l2;
    int P, B, N;
};

// pair j of the enumeration (0,1) (0,2) .. (0,P-1) (1,2) .. -> (p, q), and back
HD_DEVINL void dv_pair_of(int j, int P, int& p, int& q) {
    p = 0;
    while (j >= P - 1 - p) { j -= P - 1 - p; ++p; }
    q = p + 1 + j;
}
HD_DEVINL int dv_pair_index(int p, int q, int P) { return p * (2 * P - p - 1) / 2 + (q - p - 1); }

HD_DEVINL bool dv_finite3(const float* v) { return fabsf(v[0]) < HUGE_VALF && fabsf(v[1]) < HUGE_VALF && fabsf(v[2]) < HUGE_VALF; }

// The fit of rows xp, xq [N][3] (data units; global memory or LDS) under the masks mp, mq into F [DV_REC]; returns d2 (NaN when the
// pair contributes nothing, then F[10] = F[11] = 0).  One thread, sums over i = 0 .. N - 1 in that order.
HD_DEVINL double dv_pair_fit(const float* xp, const float* xq, const uint8_t* mp, const uint8_t* mq, int N, double inv_l2, double* F) {
    double n = 0.0, s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool bad = false;
    for (int i = 0; i < N; ++i) {
        if (!mp[i] || !mq[i]) continue;
        if (!dv_finite3(xp + 3 * i) || !dv_finite3(xq + 3 * i)) { bad = true; continue; }
        n += 1.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) { s[c] += (double)xp[3 * i + c]; s[3 + c] += (double)xq[3 * i + c]; }
    }
#pragma unroll
    for (int j = 0; j < DV_REC; ++j) F[j] = 0.0;
    F[0] = 1.0;
    if (bad || !(n > 1.0)) return NAN;
    double c[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) c[j] = s[j] / n;
    double S[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < N; ++i) {
        if (!mp[i] || !mq[i]) continue;
        const double a[3] = {(double)xp[3 * i] - c[0], (double)xp[3 * i + 1] - c[1], (double)xp[3 * i + 2] - c[2]};
        const double b[3] = {(double)xq[3 * i] - c[3], (double)xq[3 * i + 1] - c[4], (double)xq[3 * i + 2] - c[5]};
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
            for (int v = 0; v < 3; ++v) S[3 * u + v] += a[u] * b[v];
    }
    double q[4], R[9];
    kabsch_quaternion(S, q);
    kb_quat_matrix(q, R);
    double ss = 0.0;
    for (int i = 0; i < N; ++i) {
        if (!mp[i] || !mq[i]) continue;
        const double b[3] = {(double)xq[3 * i] - c[3], (double)xq[3 * i + 1] - c[4], (double)xq[3 * i + 2] - c[5]};
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const double r = ((double)xp[3 * i + u] - c[u]) - ((R[3 * u] * b[0] + R[3 * u + 1] * b[1]) + R[3 * u + 2] * b[2]);
            ss += r * r;
        }
    }
    const double d2 = ss / n;
#pragma unroll
    for (int j = 0; j < 4; ++j) F[j] = q[j];
#pragma unroll
    for (int j = 0; j < 6; ++j) F[4 + j] = c[j];
    F[10] = exp(-0.5 * d2 * inv_l2);
    F[11] = n;
    return d2;
}

// Dynamic LDS: P * N * 3 floats (x^0 of the group's rows), then - 8-byte aligned - P (P - 1) / 2 * DV_REC doubles (the pair records).
__global__ __launch_bounds__(256) void k_diverse_eps(DiverseArgs a) {
    extern __shared__ double dv_lds[];
    __shared__ double dv_mean[DV_MAX_P * 3];
    const int tid = threadIdx.x, g = blockIdx.x;
    const int N = a.N, D = a.D, P = a.P, total = P * N * D, PN = P * N;
    const size_t base = (size_t)g * total;
    const float* z = a.z + base;
    const float* eps = a.eps + base;
    float* out = a.out + base;
    const uint8_t* nm = a.nm + (size_t)g * PN;
    if (out != eps)
        for (int e = tid; e < total; e += 256) out[e] = eps[e];
    const int k = a.step_ptr ? *a.step_ptr : a.k;
    const float* row = a.rows ? a.rows + (size_t)k * 4 : a.row;
    const float al = row[0], sg = row[1], lam = row[2], clip = row[3];
    const double sl = (double)a.scale[a.scale_rows == 1 ? 0 : g] * (double)lam;
    if (sl == 0.0) return;                             // uniform over the workgroup: nothing (more) is written
    float* xs = (float*)dv_lds;                        // [P][N][3]
    double* rec = dv_lds + (PN * 3 + 1) / 2;           // [pairs][DV_REC]
    // x^0 with the operations and the order of k_chain_frame<1>: the bits record="x0" shows
    const float ra = __fdiv_rn(1.f, al);
    for (int e = tid; e < 3 * PN; e += 256) {
        const int i = e / 3, c = e - 3 * i;            // i: (row, node)
        const size_t o = (size_t)i * D + c;
        xs[e] = __fmul_rn(__fmul_rn(ra, __fsub_rn(z[o], __fmul_rn(sg, eps[o]))), a.nv0);
    }
    __syncthreads();
    const int pairs = P * (P - 1) / 2;
    for (int j = 4 * (tid & 63) + (tid >> 6); j < pairs; j += 256) {
        int p, q;
        dv_pair_of(j, P, p, q);
        dv_pair_fit(xs + (size_t)p * N * 3, xs + (size_t)q * N * 3, nm + (size_t)p * N, nm + (size_t)q * N, N, a.inv_l2, rec + (size_t)j * DV_REC);
    }
    __syncthreads();
    double* step = a.step + (size_t)g * PN * 3;
    const bool clips = clip - clip == 0.f;             // finite
    const double kl = a.kappa * a.inv_l2;
    for (int e = tid; e < PN; e += 256) {
        if (!nm[e]) continue;
        const int p = e / N, i = e - p * N;
        const float* xi = xs + (size_t)e * 3;
        double gr[3] = {0.0, 0.0, 0.0};
        for (int q = 0; q < P; ++q) {                  // the partners in ascending order
            if (q == p || !nm[(size_t)q * N + i]) continue;
            const double* F = rec + (size_t)(p < q ? dv_pair_index(p, q, P) : dv_pair_index(q, p, P)) * DV_REC;
            if (!(F[11] > 0.0)) continue;
            const float* xo = xs + ((size_t)q * N + i) * 3;
            const double qq[4] = {F[0], F[1], F[2], F[3]};
            double R[9], r[3];
            kb_quat_matrix(qq, R);
            if (p < q) {                               // this row is the pair's first: r = (x_p - c_p) - R (x_q - c_q)
                const double b[3] = {(double)xo[0] - F[7], (double)xo[1] - F[8], (double)xo[2] - F[9]};
#pragma unroll
                for (int u = 0; u < 3; ++u)
                    r[u] = ((double)xi[u] - F[4 + u]) - ((R[3 * u] * b[0] + R[3 * u + 1] * b[1]) + R[3 * u + 2] * b[2]);
            } else {                                   // its second: r = (x_q - c_q) - R^T (x_p - c_p)
                const double b[3] = {(double)xo[0] - F[4], (double)xo[1] - F[5], (double)xo[2] - F[6]};
#pragma unroll
                for (int u = 0; u < 3; ++u)
                    r[u] = ((double)xi[u] - F[7 + u]) - ((R[u] * b[0] + R[3 + u] * b[1]) + R[6 + u] * b[2]);
            }
            const double w = F[10] / F[11];
            gr[0] += w * r[0]; gr[1] += w * r[1]; gr[2] += w * r[2];
        }
        double d0 = sl * (-kl * gr[0]), d1 = sl * (-kl * gr[1]), d2 = sl * (-kl * gr[2]);
        if (clips) {
            const double len = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
            if (len > (double)clip) { const double f = (double)clip / len; d0 *= f; d1 *= f; d2 *= f; }
        }
        step[3 * e] = d0; step[3 * e + 1] = d1; step[3 * e + 2] = d2;
    }
    __syncthreads();                                   // the steps of this group are in memory for every thread of the workgroup
    if (tid < 3 * P) {                                 // the mean step of row p, component c, over its valid nodes
        const int p = tid / 3, c = tid - 3 * p;
        double s = 0.0, n = 0.0;
        for (int i = 0; i < N; ++i) {
            if (!nm[(size_t)p * N + i]) continue;
            s += step[((size_t)p * N + i) * 3 + c]; n += 1.0;
        }
        dv_mean[tid] = n > 0.0 ? s / n : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < 3 * PN; e += 256) {
        const int i = e / 3, c = e - 3 * i;
        if (!nm[i]) continue;
        const double dl = step[e] - dv_mean[(i / N) * 3 + c];
        if (dl == 0.0) continue;                       // an unmoved entry keeps its bits (-0 included)
        const size_t o = (size_t)i * D + c;
        out[o] = (float)((double)eps[o] + dl);
    }
}

// Phi [G] and the aligned RMSD matrix [G][P][P] (symmetric, zero diagonal, NaN for a pair that contributes nothing) of positions x.
__global__ __launch_bounds__(256) void k_diverse_energy(DiverseEnergyArgs a) {
    __shared__ double dv_e[DV_MAX_P * (DV_MAX_P - 1) / 2];
    const int tid = threadIdx.x, g = blockIdx.x;
    const int N = a.N, P = a.P, pairs = P * (P - 1) / 2;
    const float* x = a.x + (size_t)g * P * N * 3;
    const uint8_t* nm = a.nm + (size_t)g * P * N;
    double* rm = a.rmsd ? a.rmsd + (size_t)g * P * P : nullptr;
    for (int j = 4 * (tid & 63) + (tid >> 6); j < pairs; j += 256) {
        int p, q;
        dv_pair_of(j, P, p, q);
        double F[DV_REC];
        const double d2 = dv_pair_fit(x + (size_t)p * N * 3, x + (size_t)q * N * 3, nm + (size_t)p * N, nm + (size_t)q * N, N, a.inv_l2, F);
        dv_e[j] = F[10];
        if (rm) {
            const double d = F[11] > 0.0 ? sqrt(d2) : NAN;
            rm[p * P + q] = d; rm[q * P + p] = d;
        }
    }
    if (rm && tid < P) rm[tid * P + tid] = 0.0;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int j = 0; j < pairs; ++j) s += dv_e[j];  // pairs in ascending order
        a.phi[g] = a.kappa * s;
    }
}
