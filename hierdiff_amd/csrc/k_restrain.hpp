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
// TEMPLATES (hd_restraint_templates, hd_restraint_template_energy; k_restrain_eps<F, true>): up to HD_MAX_TEMPLATES rigid templates.
// Template t: rows (i_m, y_m, w_m) in idx [rows][NT][M] and f [rows][NT][M][4], geom [NT][2] = (k, fit: 0 rigid, 1 translation).  A row
// is active when 0 <= i_m < N, node i_m is valid and w_m > 0.  Over the active rows, in double (rs_template_fit):
//   W = sum w,  c_x = sum w x_i / W,  c_y = sum w y / W,  S = sum w (x_i - c_x)(y - c_y)^T,  R = argmax_{SO(3)} tr(R^T S) (k_kabsch.hpp;
//   translation: I),  r_m = (x_i - c_x) - R (y_m - c_y),  U_tpl = 1/2 k sum w |r|^2,  dU/dx_i += k w r_m (exact: R maximises, sum w r = 0)
// Two strided double sums per template (the centroids, then S from the centred values) with guide_block_sum, so every order depends
// on (N, M) alone; thread 64 t then solves template t - the four waves solve up to four templates side by side - and leaves
// (R, c_x, c_y, k, W) in LDS for the gather: lane l of a node's group takes the rows l, l + G, ... that name the node, behind the fields.
// W = 0, fewer than two active rows, or a non-finite active coordinate: the template contributes nothing to the molecule.  A template
// carries its own frame: it never sees tau; in the known frame rows on fixed nodes take part in the fit, only free nodes gather.
#pragma once
#include "common.hpp"
#include "k_guide.hpp"
#include "k_kabsch.hpp"

#define RS_GROUP 16
#ifndef HD_MAX_FIELDS
#define HD_MAX_FIELDS 8
#endif
#ifndef HD_MAX_TEMPLATES
#define HD_MAX_TEMPLATES 4
#endif
#define RS_FIT 19           // doubles of LDS per template: R [9], c_x [3], c_y [3], k, W (0: contributes nothing), U_tpl, sum w |r|^2

struct TemplateTables {
    const int* idx;         // [rows][NT][M]
    const float* f;         // [rows][NT][M][4] = (y, w)
    const float* geom;      // [NT][2] = (k, fit)
    int rows, NT, M;        // NT == 0: none, nothing above is read
};

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
    // TPL only, behind everything the other instantiations read
    TemplateTables tp;
};

struct TemplateEnergyArgs {
    const float* x;         // [B][N][3] positions in data units
    const uint8_t* nm;
    TemplateTables tp;
    double* out;            // [B][NT] U_tpl
    double* fit16;          // [B][NT][16] (R row-major, c_x, c_y, rmsd); null: not wanted
    int B, N;
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

HD_DEVINL bool rs_tpl_active(int i, float w, const uint8_t* nm, int N) { return i >= 0 && i < N && nm[i] && w > 0.f; }

// The fits of the molecule b's templates at positions x [N][3] (data units; global memory or LDS) into fit [NT][RS_FIT] (LDS), visible
// to every thread on return.  `red`: 4 * 9 doubles of LDS.  Every branch around a barrier is uniform over the workgroup.
HD_DEVINL void rs_template_fit(const TemplateTables& tt, int b, const float* x, const uint8_t* nm, int N, double* red, double* fit, int tid) {
    double Sk[9], ck[8];                               // of template t, kept by thread 64 t: S, (c_x, c_y), k, W
#pragma unroll
    for (int j = 0; j < 9; ++j) Sk[j] = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) ck[j] = 0.0;
    for (int t = 0; t < tt.NT; ++t) {
        const size_t row = ((size_t)(tt.rows == 1 ? 0 : b) * tt.NT + t) * tt.M;
        double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // W, sum w x, sum w y, active rows, non-finite active rows
        for (int m = tid; m < tt.M; m += 256) {
            const float* f = tt.f + (row + m) * 4;
            const int i = tt.idx[row + m];
            if (!rs_tpl_active(i, f[3], nm, N)) continue;
            const double w = (double)f[3], x0 = (double)x[3 * i], x1 = (double)x[3 * i + 1], x2 = (double)x[3 * i + 2];
            s[7] += 1.0;
            if (!(fabs(x0) < HUGE_VAL && fabs(x1) < HUGE_VAL && fabs(x2) < HUGE_VAL)) { s[8] += 1.0; continue; }
            s[0] += w;
            s[1] += w * x0; s[2] += w * x1; s[3] += w * x2;
            s[4] += w * (double)f[0]; s[5] += w * (double)f[1]; s[6] += w * (double)f[2];
        }
        guide_block_sum<9>(s, red, tid);
        const bool live = s[0] > 0.0 && s[7] >= 2.0 && s[8] == 0.0;
        double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        double S[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (live) {
#pragma unroll
            for (int j = 0; j < 6; ++j) c[j] = s[1 + j] / s[0];
            for (int m = tid; m < tt.M; m += 256) {
                const float* f = tt.f + (row + m) * 4;
                const int i = tt.idx[row + m];
                if (!rs_tpl_active(i, f[3], nm, N)) continue;
                const double w = (double)f[3];
                const double xp[3] = {(double)x[3 * i] - c[0], (double)x[3 * i + 1] - c[1], (double)x[3 * i + 2] - c[2]};
                const double yp[3] = {(double)f[0] - c[3], (double)f[1] - c[4], (double)f[2] - c[5]};
#pragma unroll
                for (int p = 0; p < 3; ++p)
#pragma unroll
                    for (int q = 0; q < 3; ++q) S[3 * p + q] += w * xp[p] * yp[q];
            }
            guide_block_sum<9>(S, red, tid);
        }
        if (tid == 64 * t) {
#pragma unroll
            for (int j = 0; j < 9; ++j) Sk[j] = S[j];
#pragma unroll
            for (int j = 0; j < 6; ++j) ck[j] = c[j];
            ck[6] = (double)tt.geom[2 * t];
            ck[7] = live ? s[0] : 0.0;
        }
    }
    const int t = tid >> 6;
    if ((tid & 63) == 0 && t < tt.NT) {
        double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
        if (ck[7] > 0.0 && tt.geom[2 * t + 1] == 0.f) kabsch_rotation(Sk, R);
        double* F = fit + t * RS_FIT;
#pragma unroll
        for (int j = 0; j < 9; ++j) F[j] = R[j];
#pragma unroll
        for (int j = 0; j < 8; ++j) F[9 + j] = ck[j];
        F[17] = 0.0; F[18] = 0.0;
    }
    __syncthreads();
}

// r_m = (x_i - c_x) - R (y_m - c_y) of one row on node i under the fit F.
HD_DEVINL void rs_tpl_residual(const double* F, const float* x, int i, const float* f, double (&r)[3]) {
    const double yp[3] = {(double)f[0] - F[12], (double)f[1] - F[13], (double)f[2] - F[14]};
#pragma unroll
    for (int c = 0; c < 3; ++c)
        r[c] = ((double)x[3 * i + c] - F[9 + c]) - ((F[3 * c] * yp[0] + F[3 * c + 1] * yp[1]) + F[3 * c + 2] * yp[2]);
}

// lane `l` of the `G` lanes that gather the valid node i: its share of dU_tpl/dx_i into g, behind rs_node_grad.
HD_DEVINL void rs_template_grad(const TemplateTables& tt, int b, const float* x, const double* fit, int i, int l, int G, double (&g)[3]) {
    for (int t = 0; t < tt.NT; ++t) {
        const double* F = fit + t * RS_FIT;
        const double k = F[15];
        if (!(k > 0.0) || !(F[16] > 0.0)) continue;
        const size_t row = ((size_t)(tt.rows == 1 ? 0 : b) * tt.NT + t) * tt.M;
        for (int m = l; m < tt.M; m += G) {
            const float* f = tt.f + (row + m) * 4;
            if (tt.idx[row + m] != i || !(f[3] > 0.f)) continue;
            double r[3];
            rs_tpl_residual(F, x, i, f, r);
            const double kw = k * (double)f[3];
            g[0] += kw * r[0]; g[1] += kw * r[1]; g[2] += kw * r[2];
        }
    }
}

// U_tpl = ((U_0 + U_1) + U_2) + U_3 of the molecule b under the fits of rs_template_fit, into every thread: per template a strided
// double sum over M, then guide_block_sum.  Thread 0 leaves U_t and sum w |r|^2 in fit[t][17], fit[t][18] (the caller's barrier makes
// them visible).  `red`: 4 doubles of LDS.
HD_DEVINL double rs_template_block(const TemplateTables& tt, int b, const float* x, const uint8_t* nm, int N, double* red, double* fit,
                                   int tid) {
    double total = 0.0;
    for (int t = 0; t < tt.NT; ++t) {
        double* F = fit + t * RS_FIT;
        if (!(F[16] > 0.0)) continue;                  // uniform over the workgroup
        const size_t row = ((size_t)(tt.rows == 1 ? 0 : b) * tt.NT + t) * tt.M;
        double q[1] = {0.0};
        for (int m = tid; m < tt.M; m += 256) {
            const float* f = tt.f + (row + m) * 4;
            const int i = tt.idx[row + m];
            if (!rs_tpl_active(i, f[3], nm, N)) continue;
            double r[3];
            rs_tpl_residual(F, x, i, f, r);
            q[0] += (double)f[3] * ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
        }
        guide_block_sum<1>(q, red, tid);
        const double U = 0.5 * F[15] * q[0];
        if (tid == 0) { F[17] = U; F[18] = q[0]; }
        total += U;
    }
    return total;
}

// Dynamic LDS: N * 3 floats (x^0 of the molecule).
template <bool FRAMED, bool TPL = false>
__global__ __launch_bounds__(256) void k_restrain_eps(RestrainArgs a) {
    extern __shared__ float rs_x[];
    __shared__ double red[4 * (TPL ? 9 : FRAMED ? 7 : 4)];
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
    double* fit = nullptr;
    if constexpr (TPL) {
        __shared__ double tp_fit[HD_MAX_TEMPLATES * RS_FIT];
        fit = tp_fit;
        rs_template_fit(a.tp, b, rs_x, nm, N, red, fit, tid);
    }
    double* step = a.step + (size_t)b * N * 3;
    const bool clips = clip - clip == 0.f;             // finite
    const int l = tid & (RS_GROUP - 1), grp = tid / RS_GROUP;
    for (int i0 = 0; i0 < N; i0 += 256 / RS_GROUP) {   // uniform trip count: the shuffles below see whole groups
        const int i = i0 + grp;
        const bool on = i < N && nm[i];
        double g[3] = {0.0, 0.0, 0.0};
        if constexpr (FRAMED) {
            if (on && !(fixed && fixed[i])) {
                rs_node_grad(a.t, b, rs_x, nm, N, i, l, RS_GROUP, g, tau);
                if constexpr (TPL) rs_template_grad(a.tp, b, rs_x, fit, i, l, RS_GROUP, g);
            }
        } else {
            if (on) {
                rs_node_grad(a.t, b, rs_x, nm, N, i, l, RS_GROUP, g);
                if constexpr (TPL) rs_template_grad(a.tp, b, rs_x, fit, i, l, RS_GROUP, g);
            }
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

// U_tpl [B][NT] and the fits (R, c_x, c_y, rmsd) [B][NT][16] of positions x.  A template that contributes nothing to a molecule (no
// weight, one active row, a non-finite active coordinate) reports U = 0, R = I, c_x = c_y = 0, rmsd = 0.
__global__ __launch_bounds__(256) void k_restraint_template_energy(TemplateEnergyArgs a) {
    __shared__ double red[4 * 9];
    __shared__ double fit[HD_MAX_TEMPLATES * RS_FIT];
    const int tid = threadIdx.x, b = blockIdx.x;
    const float* x = a.x + (size_t)b * a.N * 3;
    const uint8_t* nm = a.nm + (size_t)b * a.N;
    rs_template_fit(a.tp, b, x, nm, a.N, red, fit, tid);
    rs_template_block(a.tp, b, x, nm, a.N, red, fit, tid);
    __syncthreads();
    const int NT = a.tp.NT;
    if (tid < NT) a.out[(size_t)b * NT + tid] = fit[tid * RS_FIT + 17];
    if (a.fit16 && tid < NT * 16) {
        const int t = tid >> 4, j = tid & 15;
        const double* F = fit + t * RS_FIT;
        a.fit16[((size_t)b * NT + t) * 16 + j] = j < 15 ? F[j] : (F[16] > 0.0 ? sqrt(F[18] / F[16]) : 0.0);
    }
}
