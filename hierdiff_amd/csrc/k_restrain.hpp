// Restraint-guided sampling (hd_restraint_attach / hd_set_restraint / hd_restrain_eps / hd_restraint_energy; no reference
// counterpart).  Included through kernels.hpp.
//   k_restrain_eps<F>    eps_x += project(clip(s_b lambda_k dU/dx)) with U evaluated on the transition's data prediction x^0
//   k_restraint_energy<F> (U_obs, U_pair, U_anc) per molecule, in double, for given data-unit positions
// U, in data units (x = nv0 z_x, the model's frame: the centre of mass of the valid nodes at the origin), per molecule:
//   U_obs  = 1/2 sum_{i valid} sum_p k_p max(0, r_p - |x_i - y_p|)^2                    obs  [rows][P][5] = (y, r, k); r <= 0 or k <= 0: padding
//   U_pair = 1/2 sum_q k_q (max(0, d - hi)^2 + max(0, lo - d)^2),  d = |x_i - x_j|      pair_idx [rows][Q][2], pair_f [rows][Q][3] = (lo, hi, k)
//   U_anc  = 1/2 sum_a k_a max(0, |x_i - a| - r)^2                                       anc_idx [rows][A], anc_f [rows][A][5] = (a, r, k)
// rows = 1 (shared) or B.  A pair / anchor row is inactive when an index is < 0, >= N or masked in that molecule (or i == j, or
// k <= 0).  A term at distance exactly 0 has energy but no gradient.
// One workgroup (256 threads) per molecule as k_guide_combine.  The gradient of node i is gathered by ONE aligned group of
// RS_GROUP lanes: its lanes stride over the P obstacles, then the Q pairs (those that name i), then the A anchors (those that name
// i), each lane summing in double in that order; an xor butterfly inside the group, no atomics.  Node i belongs to group
// (i mod 256 / RS_GROUP) whatever B is, so the partition and the order of every sum depend on (N, P, Q, A) alone.  The mean of the
// clipped steps is a strided double sum per thread, the butterfly of a wave, then the four wave partials in a fixed tree
// (guide_block_sum).  Draws nothing.
// FRAMED (hd_restraint_frame 1, hd_restrain_eps_framed, hd_restraint_energy_framed): the tables are read in the frame of the known
// fragments of an inpainting call.  F = the molecule's valid fixed nodes, tau = mean_F(x^0) - mean_F(nv0 known) (a strided double sum
// per thread, then guide_block_sum: the order depends on N alone); obstacle and anchor centres are y + tau (added in double, x^0 is not
// rounded again), pairs do not see tau.  Fixed nodes gather nothing - their step is 0, the block is the frame - and receive -mean like
// every valid node, so eps_x stays mean-free and a free node moves relative to the block by its own step.  No fixed node: tau = 0 and
// the molecule's bits are those of the plain update.
// FIELDS (hd_restraint_fields, hd_restraint_field_energy[_framed]): up to HD_MAX_FIELDS scalar potentials on regular lattices, read by
// trilinear interpolation.  Field f: values v [n0][n1][n2] fp32 (last axis fastest), geom = (o[3], h[3], k, wall), weights w [rows][NF][N].
// For a valid node at p = x - tau (tau = 0 in the model's frame), per axis c, in double:
//   u = (p - o) / h,  ub = min(max(u, 0), n - 1),  cell = min((int)floor(ub), n - 2),  t = ub - cell,  out = (u - ub) h
//   E = k w_i (V + 1/2 wall sum_c out_c^2),  V the trilinear interpolant of the cell's 8 corners at t
//   dE/dx_c = k w_i ([0 <= u_c <= n_c - 1] dV/dt_c / h_c + wall out_c)
// On an interior lattice plane the gradient is the right-hand cell's, at u = n - 1 the last cell's with t = 1; outside the box an axis
// contributes only the wall.  A node with a non-finite coordinate contributes nothing (only a clamped, finite value becomes an int).
// k w_i <= 0: the term is skipped.  The 8 corners are plain global loads; lane l of a node's group takes the fields l, l + G, ...
// behind the anchors; the energy U_fld is a strided double sum over N * NF, then guide_block_sum.  In the known frame the field sees
// tau, only free nodes gather a gradient, and the energy sums over all valid nodes.
#pragma once
#include "common.hpp"
#include "k_guide.hpp"

#define RS_GROUP 16
#ifndef HD_MAX_FIELDS
#define HD_MAX_FIELDS 8
#endif

struct RestraintTables {
    const float* obs;       // [obs_rows][P][5]
    const int* pair_idx;    // [pair_rows][Q][2]
    const float* pair_f;    // [pair_rows][Q][3]
    const int* anc_idx;     // [anc_rows][A]
    const float* anc_f;     // [anc_rows][A][5]
    int obs_rows, P, pair_rows, Q, anc_rows, A;
    // fields (behind the three tables; NF == 0: none, nothing below is read)
    const float* fld_v;         // the value pool; field f is fld_v + fld_off[f], [n0][n1][n2]
    const long long* fld_off;   // [NF + 1]
    const int* fld_dims;        // [NF][3]
    const float* fld_geom;      // [NF][8] = (o, h, k, wall)
    const float* fld_w;         // [fld_w_rows][NF][N]
    int fld_w_rows, NF;
};

struct RestrainArgs {
    const float* z;         // [B][N][D] z_t
    const float* eps;       // [B][N][D] network output
    float* out;             // [B][N][D]; may be eps itself (then only the x columns of valid nodes are written)
    const uint8_t* nm;      // [B*N] node mask bytes
    RestraintTables t;
    const float* scale;     // [scale_rows] s_b, scale_rows = 1 (shared) or B
    const float* rows;      // device [K][4] {alpha_t, sigma_t, lambda_k, clip_k} (path loop); null: `row`
    float row[4];
    const int* step_ptr;    // device-side path position (graph replay); null: `k`
    int k;
    double* step;           // [B][N][3] scratch: the clipped steps before the projection
    float nv0;
    int scale_rows, B, N, D;
    // FRAMED only, behind everything the plain kernel reads so that its argument offsets - and with them its code - stay what they were
    const uint8_t* fixed;   // [B*N] fixed mask bytes
    const float* known;     // [B][N][D] normalised known values (the x columns are read)
};

struct RestraintEnergyArgs {
    const float* x;         // [B][N][3] positions in data units
    const uint8_t* nm;
    RestraintTables t;
    double* out;            // [B][3] (U_obs, U_pair, U_anc)
    int B, N;
    // FRAMED only (behind the plain kernel's arguments, as in RestrainArgs)
    const uint8_t* fixed;   // [B*N] fixed mask bytes
    const float* x_known;   // [B][N][3] known positions, data units
    double* shift;          // [B][3] tau (null: not wanted)
};

// One obstacle on the offset u = x_i - y at distance d: the energy, and in `c` the factor with dU/dx_i = c u.
HD_DEVINL double rs_obs_term(double d, double r, double k, double& c) {
    c = 0.0;
    if (!(d < r)) return 0.0;
    const double v = r - d;
    if (d > 0.0) c = -k * v / d;
    return 0.5 * k * v * v;
}

// A flat-bottomed distance term (pairs: [lo, hi]; anchors: lo = -1, hi = r) at distance d; dU/du = c u for the offset u.
HD_DEVINL double rs_band_term(double d, double lo, double hi, double k, double& c) {
    c = 0.0;
    double v;
    if (d > hi) v = d - hi;
    else if (d < lo) v = d - lo;
    else return 0.0;
    if (d > 0.0) c = k * v / d;
    return 0.5 * k * v * v;
}

HD_DEVINL double rs_dist(const float* x, int i, double yx, double yy, double yz, double (&u)[3]) {
    u[0] = (double)x[3 * i] - yx; u[1] = (double)x[3 * i + 1] - yy; u[2] = (double)x[3 * i + 2] - yz;
    return sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
}

HD_DEVINL bool rs_pair_active(const int* pi, const float* pf, const uint8_t* nm, int N, int& i, int& j) {
    i = pi[0]; j = pi[1];
    return i >= 0 && j >= 0 && i < N && j < N && i != j && nm[i] && nm[j] && pf[2] > 0.f;
}

// A translation of the obstacle and anchor centres (`on` false: none), by value so that it lives in registers.
struct RsOffset {
    double x, y, z;
    bool on;
};
#define RS_NO_OFFSET RsOffset{0.0, 0.0, 0.0, false}

// One field at p (data units, the field's frame): false for a non-finite coordinate; else V + 1/2 wall |out|^2 into e and its gradient
// into dg (both without the factor k w_i).  v: the lattice [n0][n1][n2], ge = (o, h, k, wall).
HD_DEVINL bool rs_field_term(const float* v, const int* n, const float* ge, const double (&p)[3], double& e, double (&dg)[3]) {
    double t[3], out[3], h[3];
    int cell[3];
    bool in[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        h[c] = (double)ge[3 + c];
        const double u = (p[c] - (double)ge[c]) / h[c];
        if (!(fabs(u) < HUGE_VAL)) return false;       // inf or NaN: never converted to int
        const double top = (double)(n[c] - 1);
        const double ub = fmin(fmax(u, 0.0), top);
        const int ce = (int)floor(ub);
        cell[c] = ce < n[c] - 2 ? ce : n[c] - 2;
        t[c] = ub - (double)cell[c];
        out[c] = (u - ub) * h[c];
        in[c] = u >= 0.0 && u <= top;
    }
    const size_t s1 = (size_t)n[2], s0 = (size_t)n[1] * s1;
    const float* q = v + (size_t)cell[0] * s0 + (size_t)cell[1] * s1 + (size_t)cell[2];
    const double w0[2] = {1.0 - t[0], t[0]}, w1[2] = {1.0 - t[1], t[1]}, w2[2] = {1.0 - t[2], t[2]};
    double V = 0.0, d0 = 0.0, d1 = 0.0, d2 = 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const double val = (double)q[a * s0 + b * s1 + c];
                V += val * w0[a] * w1[b] * w2[c];
                d0 += (a ? val : -val) * w1[b] * w2[c];
                d1 += (b ? val : -val) * w0[a] * w2[c];
                d2 += (c ? val : -val) * w0[a] * w1[b];
            }
    const double wall = (double)ge[7];
    e = V + 0.5 * wall * (out[0] * out[0] + out[1] * out[1] + out[2] * out[2]);
    dg[0] = (in[0] ? d0 / h[0] : 0.0) + wall * out[0];
    dg[1] = (in[1] ? d1 / h[1] : 0.0) + wall * out[1];
    dg[2] = (in[2] ? d2 / h[2] : 0.0) + wall * out[2];
    return true;
}

// k w_i of field f on node i of molecule b
HD_DEVINL double rs_field_kw(const RestraintTables& t, int b, int N, int f, int i) {
    return (double)t.fld_geom[f * 8 + 6] * (double)t.fld_w[((size_t)(t.fld_w_rows == 1 ? 0 : b) * t.NF + f) * N + i];
}

// lane `l` of the `G` lanes that gather node i: its share of dU/dx_i into g (x: the molecule's positions, data units).  `off`: the
// translation of the obstacle and anchor centres.
HD_DEVINL void rs_node_grad(const RestraintTables& t, int b, const float* x, const uint8_t* nm, int N, int i, int l, int G,
                            double (&g)[3], const RsOffset off = RS_NO_OFFSET) {
    double u[3], c;
    const float* obs = t.obs + (size_t)(t.obs_rows == 1 ? 0 : b) * t.P * 5;
    for (int p = l; p < t.P; p += G) {
        const float* o = obs + (size_t)p * 5;
        if (!(o[3] > 0.f) || !(o[4] > 0.f)) continue;
        const double d = off.on ? rs_dist(x, i, (double)o[0] + off.x, (double)o[1] + off.y, (double)o[2] + off.z, u)
                             : rs_dist(x, i, (double)o[0], (double)o[1], (double)o[2], u);
        rs_obs_term(d, (double)o[3], (double)o[4], c);
        g[0] += c * u[0]; g[1] += c * u[1]; g[2] += c * u[2];
    }
    const size_t prow = (size_t)(t.pair_rows == 1 ? 0 : b) * t.Q;
    for (int q = l; q < t.Q; q += G) {
        const float* pf = t.pair_f + (prow + q) * 3;
        int a, c2;
        if (!rs_pair_active(t.pair_idx + (prow + q) * 2, pf, nm, N, a, c2)) continue;
        if (a != i && c2 != i) continue;
        const int o = a == i ? c2 : a;
        const double d = rs_dist(x, i, (double)x[3 * o], (double)x[3 * o + 1], (double)x[3 * o + 2], u);
        rs_band_term(d, (double)pf[0], (double)pf[1], (double)pf[2], c);
        g[0] += c * u[0]; g[1] += c * u[1]; g[2] += c * u[2];
    }
    const size_t arow = (size_t)(t.anc_rows == 1 ? 0 : b) * t.A;
    for (int a = l; a < t.A; a += G) {
        const float* af = t.anc_f + (arow + a) * 5;
        if (t.anc_idx[arow + a] != i || !(af[4] > 0.f) || !(af[3] >= 0.f)) continue;
        const double d = off.on ? rs_dist(x, i, (double)af[0] + off.x, (double)af[1] + off.y, (double)af[2] + off.z, u)
                             : rs_dist(x, i, (double)af[0], (double)af[1], (double)af[2], u);
        rs_band_term(d, -1.0, (double)af[3], (double)af[4], c);
        g[0] += c * u[0]; g[1] += c * u[1]; g[2] += c * u[2];
    }
    for (int f = l; f < t.NF; f += G) {
        const double kw = rs_field_kw(t, b, N, f, i);
        if (!(kw > 0.0)) continue;
        const double p[3] = {off.on ? (double)x[3 * i] - off.x : (double)x[3 * i], off.on ? (double)x[3 * i + 1] - off.y : (double)x[3 * i + 1],
                             off.on ? (double)x[3 * i + 2] - off.z : (double)x[3 * i + 2]};
        double e, dg[3];
        if (!rs_field_term(t.fld_v + t.fld_off[f], t.fld_dims + f * 3, t.fld_geom + f * 8, p, e, dg)) continue;
        g[0] += kw * dg[0]; g[1] += kw * dg[1]; g[2] += kw * dg[2];
    }
}

// tau of molecule b into every thread (0 and off without valid fixed nodes): pos [N][stride] positions in data units, known
// [N][kstride] times ks.  `red`: 4 * 7 doubles of LDS.
HD_DEVINL bool rs_frame_shift(const float* pos, int stride, const float* known, int kstride, double ks, const uint8_t* nm,
                              const uint8_t* fixed, int N, double* red, int tid, RsOffset& tau) {
    double f[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // nf, sum_F pos, sum_F known
    for (int i = tid; i < N; i += 256) {
        if (!nm[i] || !fixed[i]) continue;
        f[0] += 1.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            f[1 + c] += (double)pos[(size_t)i * stride + c];
            f[4 + c] += ks * (double)known[(size_t)i * kstride + c];
        }
    }
    guide_block_sum<7>(f, red, tid);
    const bool any = f[0] > 0.0;
    tau.x = any ? f[1] / f[0] - f[4] / f[0] : 0.0;
    tau.y = any ? f[2] / f[0] - f[5] / f[0] : 0.0;
    tau.z = any ? f[3] / f[0] - f[6] / f[0] : 0.0;
    tau.on = any;
    return any;
}

// Dynamic LDS: N * 3 floats (x^0 of the molecule).
template <bool FRAMED>
__global__ __launch_bounds__(256) void k_restrain_eps(RestrainArgs a) {
    extern __shared__ float rs_x[];
    __shared__ double red[4 * (FRAMED ? 7 : 4)];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int N = a.N, D = a.D, total = N * D;
    const size_t base = (size_t)b * total;
    const float* z = a.z + base;
    const float* eps = a.eps + base;
    float* out = a.out + base;
    const uint8_t* nm = a.nm + (size_t)b * N;
    if (out != eps)
        for (int e = tid; e < total; e += 256) out[e] = eps[e];
    const int k = a.step_ptr ? *a.step_ptr : a.k;
    const float* row = a.rows ? a.rows + (size_t)k * 4 : a.row;
    const float al = row[0], sg = row[1], lam = row[2], clip = row[3];
    const double sl = (double)a.scale[a.scale_rows == 1 ? 0 : b] * (double)lam;
    if (sl == 0.0) return;                             // uniform over the workgroup: nothing (more) is written
    // x^0 with the operations and the order of k_chain_frame<1>: the bits record="x0" shows
    const float ra = __fdiv_rn(1.f, al);
    for (int e = tid; e < 3 * N; e += 256) {
        const int i = e / 3, c = e - 3 * i;
        const size_t o = (size_t)i * D + c;
        rs_x[e] = __fmul_rn(__fmul_rn(ra, __fsub_rn(z[o], __fmul_rn(sg, eps[o]))), a.nv0);
    }
    __syncthreads();
    RsOffset tau = RS_NO_OFFSET;
    const uint8_t* fixed = nullptr;                    // null: every valid node is free
    if constexpr (FRAMED) {
        if (rs_frame_shift(rs_x, 3, a.known + base, D, (double)a.nv0, nm, a.fixed + (size_t)b * N, N, red, tid, tau))
            fixed = a.fixed + (size_t)b * N;           // uniform over the workgroup
    }
    double* step = a.step + (size_t)b * N * 3;
    const bool clips = clip - clip == 0.f;             // finite
    const int l = tid & (RS_GROUP - 1), grp = tid / RS_GROUP;
    for (int i0 = 0; i0 < N; i0 += 256 / RS_GROUP) {   // uniform trip count: the shuffles below see whole groups
        const int i = i0 + grp;
        const bool on = i < N && nm[i];
        double g[3] = {0.0, 0.0, 0.0};
        if constexpr (FRAMED) {
            if (on && !(fixed && fixed[i])) rs_node_grad(a.t, b, rs_x, nm, N, i, l, RS_GROUP, g, tau);
        } else {
            if (on) rs_node_grad(a.t, b, rs_x, nm, N, i, l, RS_GROUP, g);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int o = RS_GROUP / 2; o > 0; o >>= 1) g[c] += __shfl_xor(g[c], o);
        if (on && l == 0) {
            double d0 = sl * g[0], d1 = sl * g[1], d2 = sl * g[2];
            if (clips) {
                const double len = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
                if (len > (double)clip) { const double f = (double)clip / len; d0 *= f; d1 *= f; d2 *= f; }
            }
            step[3 * i] = d0; step[3 * i + 1] = d1; step[3 * i + 2] = d2;
        }
    }
    __syncthreads();                                   // the steps of this molecule are in memory for every thread of the workgroup
    double s[4] = {0.0, 0.0, 0.0, 0.0};                // sum of the steps, valid nodes
    for (int i = tid; i < N; i += 256) {
        if (!nm[i]) continue;
        s[0] += step[3 * i]; s[1] += step[3 * i + 1]; s[2] += step[3 * i + 2]; s[3] += 1.0;
    }
    guide_block_sum<4>(s, red, tid);
    if (!(s[3] > 0.0)) return;
    const double m[3] = {s[0] / s[3], s[1] / s[3], s[2] / s[3]};
    for (int e = tid; e < 3 * N; e += 256) {
        const int i = e / 3, c = e - 3 * i;
        if (!nm[i]) continue;
        const double dl = step[e] - m[c];
        if (dl == 0.0) continue;                       // an unmoved entry keeps its bits (-0 included)
        const size_t o = (size_t)i * D + c;
        out[o] = (float)((double)eps[o] + dl);
    }
}

// U_fld of the molecule b at positions x [N][3] into every thread: a strided double sum over N * NF per thread, then guide_block_sum.
// `red`: 4 doubles of LDS.  NF == 0 (uniform): 0 without a barrier.
HD_DEVINL double rs_field_block(const RestraintTables& t, int b, const float* x, const uint8_t* nm, int N, double* red, int tid,
                                const RsOffset off = RS_NO_OFFSET) {
    if (t.NF == 0) return 0.0;
    double U[1] = {0.0};
    for (int e = tid; e < N * t.NF; e += 256) {
        const int i = e / t.NF, f = e - i * t.NF;
        if (!nm[i]) continue;
        const double kw = rs_field_kw(t, b, N, f, i);
        if (!(kw > 0.0)) continue;
        const double p[3] = {off.on ? (double)x[3 * i] - off.x : (double)x[3 * i], off.on ? (double)x[3 * i + 1] - off.y : (double)x[3 * i + 1],
                             off.on ? (double)x[3 * i + 2] - off.z : (double)x[3 * i + 2]};
        double en, dg[3];
        if (!rs_field_term(t.fld_v + t.fld_off[f], t.fld_dims + f * 3, t.fld_geom + f * 8, p, en, dg)) continue;
        U[0] += kw * en;
    }
    guide_block_sum<1>(U, red, tid);
    return U[0];
}

// (U_obs, U_pair, U_anc) of the molecule b at positions x [N][3] (data units; global memory or LDS) into U, in every thread: a strided
// double sum per thread, then guide_block_sum.  `red`: 4 * 3 doubles of LDS.  The one energy code of k_restraint_energy and k_steer_weigh.
// `off`: the translation of the obstacle and anchor centres (and of the fields' frame).  U[3] = U_fld (rs_field_block) when `fields`, else 0:
// the first three components, their loops and their reduction do not see it.
HD_DEVINL void rs_energy_block(const RestraintTables& t, int b, const float* x, const uint8_t* nm, int N, double* red, int tid,
                               double (&U4)[4], const RsOffset off = RS_NO_OFFSET, bool fields = true) {
    double u[3], c;
    double U[3];
    U[0] = 0.0; U[1] = 0.0; U[2] = 0.0;
    const float* obs = t.obs + (size_t)(t.obs_rows == 1 ? 0 : b) * t.P * 5;
    for (long long e = tid; e < (long long)N * t.P; e += 256) {
        const int i = (int)(e / t.P), p = (int)(e - (long long)i * t.P);
        const float* o = obs + (size_t)p * 5;
        if (!nm[i] || !(o[3] > 0.f) || !(o[4] > 0.f)) continue;
        const double d = off.on ? rs_dist(x, i, (double)o[0] + off.x, (double)o[1] + off.y, (double)o[2] + off.z, u)
                             : rs_dist(x, i, (double)o[0], (double)o[1], (double)o[2], u);
        U[0] += rs_obs_term(d, (double)o[3], (double)o[4], c);
    }
    const size_t prow = (size_t)(t.pair_rows == 1 ? 0 : b) * t.Q;
    for (int q = tid; q < t.Q; q += 256) {
        const float* pf = t.pair_f + (prow + q) * 3;
        int i, j;
        if (!rs_pair_active(t.pair_idx + (prow + q) * 2, pf, nm, N, i, j)) continue;
        const double d = rs_dist(x, i, (double)x[3 * j], (double)x[3 * j + 1], (double)x[3 * j + 2], u);
        U[1] += rs_band_term(d, (double)pf[0], (double)pf[1], (double)pf[2], c);
    }
    const size_t arow = (size_t)(t.anc_rows == 1 ? 0 : b) * t.A;
    for (int q = tid; q < t.A; q += 256) {
        const float* af = t.anc_f + (arow + q) * 5;
        const int i = t.anc_idx[arow + q];
        if (i < 0 || i >= N || !nm[i] || !(af[4] > 0.f) || !(af[3] >= 0.f)) continue;
        const double d = off.on ? rs_dist(x, i, (double)af[0] + off.x, (double)af[1] + off.y, (double)af[2] + off.z, u)
                             : rs_dist(x, i, (double)af[0], (double)af[1], (double)af[2], u);
        U[2] += rs_band_term(d, -1.0, (double)af[3], (double)af[4], c);
    }
    guide_block_sum<3>(U, red, tid);
    U4[0] = U[0]; U4[1] = U[1]; U4[2] = U[2];
    U4[3] = fields ? rs_field_block(t, b, x, nm, N, red, tid, off) : 0.0;
}

template <bool FRAMED>
__global__ __launch_bounds__(256) void k_restraint_energy(RestraintEnergyArgs a) {
    __shared__ double red[4 * (FRAMED ? 7 : 3)];
    const int tid = threadIdx.x, b = blockIdx.x;
    const float* x = a.x + (size_t)b * a.N * 3;
    const uint8_t* nm = a.nm + (size_t)b * a.N;
    double U[4];
    if constexpr (FRAMED) {
        RsOffset tau;
        rs_frame_shift(x, 3, a.x_known + (size_t)b * a.N * 3, 3, 1.0, nm, a.fixed + (size_t)b * a.N, a.N, red, tid, tau);
        tau.on = true;                                  // (no fixed node: tau = 0)
        rs_energy_block(a.t, b, x, nm, a.N, red, tid, U, tau, false);
        if (a.shift && tid < 3) a.shift[(size_t)b * 3 + tid] = tid == 0 ? tau.x : tid == 1 ? tau.y : tau.z;
    } else {
        rs_energy_block(a.t, b, x, nm, a.N, red, tid, U, RS_NO_OFFSET, false);
    }
    if (tid < 3) a.out[(size_t)b * 3 + tid] = U[tid];
}

// U_fld per molecule (RestraintEnergyArgs with out [B]).
template <bool FRAMED>
__global__ __launch_bounds__(256) void k_restraint_field_energy(RestraintEnergyArgs a) {
    __shared__ double red[4 * (FRAMED ? 7 : 1)];
    const int tid = threadIdx.x, b = blockIdx.x;
    const float* x = a.x + (size_t)b * a.N * 3;
    const uint8_t* nm = a.nm + (size_t)b * a.N;
    double U;
    if constexpr (FRAMED) {
        RsOffset tau;
        rs_frame_shift(x, 3, a.x_known + (size_t)b * a.N * 3, 3, 1.0, nm, a.fixed + (size_t)b * a.N, a.N, red, tid, tau);
        tau.on = true;
        U = rs_field_block(a.t, b, x, nm, a.N, red, tid, tau);
        if (a.shift && tid < 3) a.shift[(size_t)b * 3 + tid] = tid == 0 ? tau.x : tid == 1 ? tau.y : tau.z;
    } else {
        U = rs_field_block(a.t, b, x, nm, a.N, red, tid);
    }
    if (tid == 0) a.out[b] = U;
}
