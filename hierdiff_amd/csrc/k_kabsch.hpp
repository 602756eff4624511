// The rigid-superposition solver of the template restraints (k_restrain.hpp: rs_template_fit).  Included through k_restrain.hpp.
//   kabsch_rotation   R = argmax_{R in SO(3)} tr(R^T S) for a 3x3 S = sum_m w_m x'_m y'_m^T, so that x' ~ R y'.
// Horn's quaternion form: tr(R^T S) = q^T K q for the unit quaternion q of R, with K the symmetric 4x4 matrix below, so the best q is
// the eigenvector of K's largest eigenvalue - a proper rotation (det +1) by construction, no reflection branch.  The eigenvectors come
// from a cyclic Jacobi iteration in double: KB_SWEEPS sweeps over the six pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), in that order,
// always all of them - the operations depend on S alone, never on where the molecule sits in the batch.  Every index is a compile-time
// constant, so the two 4x4 arrays live in registers.  A degenerate largest eigenvalue (R not unique) still yields an orthonormal
// eigenvector of it: some maximiser.  S = 0 yields R = I.
// Plain C++ (sqrt, fabs): a host build may include this file alone, HD_DEVINL then falls back to `inline`.
#pragma once
#include <math.h>
#ifndef HD_DEVINL
#define HD_DEVINL inline
#endif

#define KB_SWEEPS 10

// One Jacobi rotation in the (P, Q) plane: A <- J^T A J with A[P][Q] -> 0, V <- V J.
template <int P, int Q>
HD_DEVINL void kb_rotate(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));   // (|theta| = inf: t = 0)
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = c * akp - s * akq;
        A[k][Q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double apk = A[P][k], aqk = A[Q][k];
        A[P][k] = c * apk - s * aqk;
        A[Q][k] = s * apk + c * aqk;
    }
    A[P][Q] = 0.0; A[Q][P] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

// S row-major [3][3] (S[3 a + b] = sum w x'_a y'_b) -> the unit quaternion q of R (k_diverse.hpp keeps q per pair and rebuilds R).
HD_DEVINL void kabsch_quaternion(const double (&S)[9], double (&q)[4]) {
    const double xx = S[0], xy = S[1], xz = S[2], yx = S[3], yy = S[4], yz = S[5], zx = S[6], zy = S[7], zz = S[8];
    double A[4][4], V[4][4];
    A[0][0] = xx + yy + zz; A[0][1] = zy - yz;      A[0][2] = xz - zx;       A[0][3] = yx - xy;
    A[1][1] = xx - yy - zz; A[1][2] = xy + yx;      A[1][3] = zx + xz;
    A[2][2] = -xx + yy - zz; A[2][3] = yz + zy;
    A[3][3] = -xx - yy + zz;
    A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[3][0] = A[0][3]; A[2][1] = A[1][2]; A[3][1] = A[1][3]; A[3][2] = A[2][3];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < KB_SWEEPS; ++sweep) {
        kb_rotate<0, 1>(A, V); kb_rotate<0, 2>(A, V); kb_rotate<0, 3>(A, V);
        kb_rotate<1, 2>(A, V); kb_rotate<1, 3>(A, V); kb_rotate<2, 3>(A, V);
    }
    // the column of the largest eigenvalue (the first of equal ones), picked by 0 / 1 factors: a chain of selects becomes a dynamic
    // index into V in the compiler's hands, and with it private memory
    const double e0 = A[0][0], e1 = A[1][1], e2 = A[2][2], e3 = A[3][3];
    const double m1 = (e1 > e0 && e1 >= e2 && e1 >= e3) ? 1.0 : 0.0;
    const double m2 = (e2 > e0 && e2 > e1 && e2 >= e3) ? 1.0 : 0.0;
    const double m3 = (e3 > e0 && e3 > e1 && e3 > e2) ? 1.0 : 0.0;
    const double m0 = 1.0 - ((m1 + m2) + m3);
    double q0 = ((m0 * V[0][0] + m1 * V[0][1]) + m2 * V[0][2]) + m3 * V[0][3];
    double q1 = ((m0 * V[1][0] + m1 * V[1][1]) + m2 * V[1][2]) + m3 * V[1][3];
    double q2 = ((m0 * V[2][0] + m1 * V[2][1]) + m2 * V[2][2]) + m3 * V[2][3];
    double q3 = ((m0 * V[3][0] + m1 * V[3][1]) + m2 * V[3][2]) + m3 * V[3][3];
    const double n = 1.0 / sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    q[0] = q0 * n; q[1] = q1 * n; q[2] = q2 * n; q[3] = q3 * n;
}

// The rotation matrix (row-major) of the unit quaternion q.
HD_DEVINL void kb_quat_matrix(const double (&q)[4], double (&R)[9]) {
    const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    R[0] = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3; R[1] = 2.0 * (q1 * q2 - q0 * q3); R[2] = 2.0 * (q1 * q3 + q0 * q2);
    R[3] = 2.0 * (q1 * q2 + q0 * q3); R[4] = q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3; R[5] = 2.0 * (q2 * q3 - q0 * q1);
    R[6] = 2.0 * (q1 * q3 - q0 * q2); R[7] = 2.0 * (q2 * q3 + q0 * q1); R[8] = q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3;
}

// S row-major [3][3] (S[3 a + b] = sum w x'_a y'_b) -> R row-major [3][3].
HD_DEVINL void kabsch_rotation(const double (&S)[9], double (&R)[9]) {
    double q[4];
    kabsch_quaternion(S, q);
    kb_quat_matrix(q, R);
}
