// Register-level algebra of the state-space Matern GP (kernels_ss.hip): 1-D inputs, nu = 3/2 (state size D = 2) and 5/2 (D = 3).
// Sarkka & Garcia-Fernandez, Temporal Parallelization of Bayesian Smoothers (2021): the Kalman filter and the RTS smoother as two
// associative scans.  Everything here is a D x D product, solve or inverse on local arrays whose every index is a compile-time constant
// after unrolling, so an element lives in registers; symmetric matrices travel packed (upper triangle, row by row).
#pragma once
#include <cmath>

#ifndef __HIPCC__
#define __host__
#define __device__
#define __forceinline__ inline
#endif
#define SS_FN __host__ __device__ __forceinline__
#define SS_UNROLL _Pragma("unroll")

struct ss_par { double lam, sf2, R; };     // lambda = sqrt(2 nu) / l, sf^2, sn^2

SS_FN ss_par ss_make_par(const double *theta, int D) {
    ss_par p;
    p.lam = sqrt((double)(2 * D - 1)) / theta[1];
    p.sf2 = theta[0] * theta[0];
    p.R = theta[2] * theta[2];
    return p;
}

template <int D> SS_FN constexpr int ss_sidx(int i, int j) { return i <= j ? i * D - i * (i - 1) / 2 + j - i : j * D - j * (j - 1) / 2 + i - j; }

template <int D> SS_FN void ss_unpack(const double *p, double (&M)[D][D]) {
    SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) M[i][j] = p[ss_sidx<D>(i, j)]; }
}
template <int D> SS_FN void ss_pack(const double (&M)[D][D], double *p) {      // the symmetric part
    SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = i; j < D; ++j) p[ss_sidx<D>(i, j)] = i == j ? M[i][i] : 0.5 * (M[i][j] + M[j][i]); }
}
template <int D> SS_FN void ss_load(const double *p, double (&M)[D][D]) {
    SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) M[i][j] = p[i * D + j]; }
}
template <int D> SS_FN void ss_store(const double (&M)[D][D], double *p) {
    SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) p[i * D + j] = M[i][j]; }
}
// C = A B, A B^T, A^T B
template <int D> SS_FN void ss_mm(const double (&A)[D][D], const double (&B)[D][D], double (&C)[D][D]) {
    SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) {
        double s = A[i][0] * B[0][j];
        SS_UNROLL for (int k = 1; k < D; ++k) s = fma(A[i][k], B[k][j], s);
        C[i][j] = s; } }
}
template <int D> SS_FN void ss_mm_nt(const double (&A)[D][D], const double (&B)[D][D], double (&C)[D][D]) {
    SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) {
        double s = A[i][0] * B[j][0];
        SS_UNROLL for (int k = 1; k < D; ++k) s = fma(A[i][k], B[j][k], s);
        C[i][j] = s; } }
}
template <int D> SS_FN void ss_mm_tn(const double (&A)[D][D], const double (&B)[D][D], double (&C)[D][D]) {
    SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) {
        double s = A[0][i] * B[0][j];
        SS_UNROLL for (int k = 1; k < D; ++k) s = fma(A[k][i], B[k][j], s);
        C[i][j] = s; } }
}
// y = A x, A^T x
template <int D> SS_FN void ss_mv(const double (&A)[D][D], const double (&x)[D], double (&y)[D]) {
    SS_UNROLL for (int i = 0; i < D; ++i) { double s = A[i][0] * x[0]; SS_UNROLL for (int k = 1; k < D; ++k) s = fma(A[i][k], x[k], s); y[i] = s; }
}
template <int D> SS_FN void ss_mtv(const double (&A)[D][D], const double (&x)[D], double (&y)[D]) {
    SS_UNROLL for (int i = 0; i < D; ++i) { double s = A[0][i] * x[0]; SS_UNROLL for (int k = 1; k < D; ++k) s = fma(A[k][i], x[k], s); y[i] = s; }
}
// closed-form inverse (adjugate): for T = I + C J with C, J symmetric PSD det T >= 1, so no pivoting is needed
SS_FN void ss_inv(const double (&T)[2][2], double (&M)[2][2]) {
    const double r = 1.0 / (T[0][0] * T[1][1] - T[0][1] * T[1][0]);
    M[0][0] = T[1][1] * r, M[0][1] = -T[0][1] * r, M[1][0] = -T[1][0] * r, M[1][1] = T[0][0] * r;
}
SS_FN void ss_inv(const double (&T)[3][3], double (&M)[3][3]) {
    const double c00 = T[1][1] * T[2][2] - T[1][2] * T[2][1], c01 = T[1][2] * T[2][0] - T[1][0] * T[2][2], c02 = T[1][0] * T[2][1] - T[1][1] * T[2][0];
    const double r = 1.0 / (T[0][0] * c00 + T[0][1] * c01 + T[0][2] * c02);
    M[0][0] = c00 * r, M[1][0] = c01 * r, M[2][0] = c02 * r;
    M[0][1] = (T[0][2] * T[2][1] - T[0][1] * T[2][2]) * r, M[1][1] = (T[0][0] * T[2][2] - T[0][2] * T[2][0]) * r, M[2][1] = (T[0][1] * T[2][0] - T[0][0] * T[2][1]) * r;
    M[0][2] = (T[0][1] * T[1][2] - T[0][2] * T[1][1]) * r, M[1][2] = (T[0][2] * T[1][0] - T[0][0] * T[1][2]) * r, M[2][2] = (T[0][0] * T[1][1] - T[0][1] * T[1][0]) * r;
}
// X = P^-1 G for a symmetric positive definite P (its lower triangle is read): L D L^T without square roots, then D solves
template <int D> SS_FN void ss_spd_solve(const double (&P)[D][D], const double (&G)[D][D], double (&X)[D][D]) {
    double Lm[D][D], d[D];
    SS_UNROLL for (int j = 0; j < D; ++j) {
        double s = P[j][j];
        SS_UNROLL for (int k = 0; k < j; ++k) s -= Lm[j][k] * Lm[j][k] * d[k];
        d[j] = s;
        SS_UNROLL for (int i = j + 1; i < D; ++i) {
            double u = P[i][j];
            SS_UNROLL for (int k = 0; k < j; ++k) u -= Lm[i][k] * Lm[j][k] * d[k];
            Lm[i][j] = u / s;
        }
    }
    SS_UNROLL for (int c = 0; c < D; ++c) {
        double z[D];
        SS_UNROLL for (int i = 0; i < D; ++i) { double s = G[i][c]; SS_UNROLL for (int k = 0; k < i; ++k) s -= Lm[i][k] * z[k]; z[i] = s; }
        SS_UNROLL for (int i = D - 1; i >= 0; --i) { double s = z[i] / d[i]; SS_UNROLL for (int k = i + 1; k < D; ++k) s -= Lm[k][i] * X[k][c]; X[i][c] = s; }
    }
}

// transition A(dt) and process noise Q(dt) = Pinf - A Pinf A^T of one step; first: the prior N(0, Pinf) as a step with A = 0
SS_FN void ss_pinf(const ss_par &p, double (&P)[2][2]) { P[0][0] = p.sf2, P[0][1] = P[1][0] = 0.0, P[1][1] = p.lam * p.lam * p.sf2; }
SS_FN void ss_pinf(const ss_par &p, double (&P)[3][3]) {
    const double l2 = p.lam * p.lam, kap = l2 / 3.0;
    P[0][0] = p.sf2, P[0][1] = P[1][0] = 0.0, P[0][2] = P[2][0] = -kap * p.sf2;
    P[1][1] = kap * p.sf2, P[1][2] = P[2][1] = 0.0, P[2][2] = l2 * l2 * p.sf2;
}
SS_FN void ss_amat(const ss_par &p, double dt, double (&A)[2][2]) {
    const double x = p.lam * dt, e = exp(-x);
    A[0][0] = e * (1.0 + x), A[0][1] = e * dt, A[1][0] = -e * p.lam * x, A[1][1] = e * (1.0 - x);
}
SS_FN void ss_amat(const ss_par &p, double dt, double (&A)[3][3]) {
    const double l = p.lam, x = l * dt, e = exp(-x);
    A[0][0] = e * (0.5 * x * x + x + 1.0), A[0][1] = e * dt * (x + 1.0), A[0][2] = e * 0.5 * dt * dt;
    A[1][0] = -e * 0.5 * l * x * x, A[1][1] = -e * (x * x - x - 1.0), A[1][2] = -e * 0.5 * dt * (x - 2.0);
    A[2][0] = e * 0.5 * l * l * x * (x - 2.0), A[2][1] = e * l * x * (x - 3.0), A[2][2] = e * 0.5 * (x * x - 4.0 * x + 2.0);
}
template <int D> SS_FN void ss_trans(const ss_par &p, double dt, bool first, double (&A)[D][D], double (&Q)[D][D]) {
    double Pi[D][D];
    ss_pinf(p, Pi);
    if (first) {
        SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) A[i][j] = 0.0, Q[i][j] = Pi[i][j]; }
        return;
    }
    double AP[D][D], APA[D][D];
    ss_amat(p, dt, A);
    ss_mm<D>(A, Pi, AP);
    ss_mm_nt<D>(AP, A, APA);
    SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) Q[i][j] = Pi[i][j] - 0.5 * (APA[i][j] + APA[j][i]); }
}

// ---- filtering: element (A, b, C, eta, J), a (x) b with a the earlier one ---------------------------------------------------------
template <int D> struct ss_filt {
    static constexpr int NS = D * (D + 1) / 2, OA = 0, OB = D * D, OC = OB + D, OH = OC + NS, OJ = OH + D, NV = OJ + NS;
    static constexpr int STATE = OB, NSTATE = D + NS;      // (b, C): the filtered mean and covariance of a prefix
    static SS_FN void identity(double (&v)[NV]) {
        SS_UNROLL for (int i = 0; i < NV; ++i) v[i] = 0.0;
        SS_UNROLL for (int i = 0; i < D; ++i) v[OA + i * D + i] = 1.0;
    }
    static SS_FN void op(const double (&a)[NV], const double (&b)[NV], double (&o)[NV]) {
        double Ai[D][D], Aj[D][D], Ci[D][D], Cj[D][D], Ji[D][D], Jj[D][D], T[D][D], M[D][D], X[D][D], Y[D][D];
        ss_load<D>(a + OA, Ai), ss_load<D>(b + OA, Aj);
        ss_unpack<D>(a + OC, Ci), ss_unpack<D>(b + OC, Cj), ss_unpack<D>(a + OJ, Ji), ss_unpack<D>(b + OJ, Jj);
        ss_mm<D>(Ci, Jj, T);
        SS_UNROLL for (int i = 0; i < D; ++i) T[i][i] += 1.0;
        ss_inv(T, M);                                          // M = (I + C_i J_j)^-1
        double u[D], w[D], r[D];
        SS_UNROLL for (int i = 0; i < D; ++i) r[i] = b[OH + i];
        ss_mv<D>(Ci, r, u);
        SS_UNROLL for (int i = 0; i < D; ++i) u[i] += a[OB + i];              // b_i + C_i eta_j
        ss_mv<D>(M, u, w);
        ss_mv<D>(Aj, w, u);
        SS_UNROLL for (int i = 0; i < D; ++i) o[OB + i] = u[i] + b[OB + i];   // b = A_j M (b_i + C_i eta_j) + b_j
        ss_mm<D>(M, Ci, X);
        ss_mm<D>(Aj, X, Y);
        ss_mm_nt<D>(Y, Aj, X);
        SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) X[i][j] += Cj[i][j]; }
        ss_pack<D>(X, o + OC);                                 // C = A_j M C_i A_j^T + C_j
        ss_mm<D>(M, Ai, X);                                    // X = M A_i
        ss_mm<D>(Aj, X, Y);
        ss_store<D>(Y, o + OA);                                // A = A_j M A_i
        SS_UNROLL for (int i = 0; i < D; ++i) r[i] = a[OB + i];
        ss_mv<D>(Jj, r, u);
        SS_UNROLL for (int i = 0; i < D; ++i) u[i] = b[OH + i] - u[i];        // eta_j - J_j b_i
        ss_mtv<D>(X, u, w);
        SS_UNROLL for (int i = 0; i < D; ++i) o[OH + i] = w[i] + a[OH + i];   // eta = A_i^T M^T (eta_j - J_j b_i) + eta_i
        ss_mm_tn<D>(X, Jj, Y);
        ss_mm<D>(Y, Ai, T);
        SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) T[i][j] += Ji[i][j]; }
        ss_pack<D>(T, o + OJ);                                 // J = A_i^T M^T J_j A_i + J_i
    }
    // the element of one step with transition (A, Q); observed: target y with noise R.  *S: the innovation variance the element divides by
    static SS_FN void element(const double (&A)[D][D], const double (&Q)[D][D], bool observed, double y, double R, double (&v)[NV], double *S) {
        if (!observed) {
            SS_UNROLL for (int i = 0; i < NV; ++i) v[i] = 0.0;
            ss_store<D>(A, v + OA);
            ss_pack<D>(Q, v + OC);
            *S = 1.0;
            return;
        }
        const double s = Q[0][0] + R, rs = 1.0 / s;
        double K[D], X[D][D];
        SS_UNROLL for (int i = 0; i < D; ++i) K[i] = Q[i][0] * rs;
        SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) v[OA + i * D + j] = A[i][j] - K[i] * A[0][j]; }
        SS_UNROLL for (int i = 0; i < D; ++i) v[OB + i] = K[i] * y;
        SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) X[i][j] = Q[i][j] - K[i] * Q[0][j]; }
        ss_pack<D>(X, v + OC);
        SS_UNROLL for (int i = 0; i < D; ++i) v[OH + i] = A[0][i] * y * rs;
        SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = i; j < D; ++j) v[OJ + ss_sidx<D>(i, j)] = A[0][i] * A[0][j] * rs; }
        *S = s;
    }
};

// One Kalman step on the filtered moments (m, P) -> (m, P) of the next step; returns the step's term of the LML (0 if unobserved) and
// *S = the predicted innovation variance P^-_00 + R
template <int D> SS_FN double ss_kalman_step(const double (&A)[D][D], const double (&Q)[D][D], bool observed, double y, double R,
                                             double (&m)[D], double (&P)[D][D], double *S) {
    double mp[D], X[D][D], Pp[D][D];
    ss_mv<D>(A, m, mp);
    ss_mm<D>(A, P, X);
    ss_mm_nt<D>(X, A, Pp);
    SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) P[i][j] = 0.5 * (Pp[i][j] + Pp[j][i]) + Q[i][j]; }
    SS_UNROLL for (int i = 0; i < D; ++i) m[i] = mp[i];
    *S = 1.0;
    if (!observed) return 0.0;
    const double s = P[0][0] + R, rs = 1.0 / s, v = y - m[0];
    double K[D];
    SS_UNROLL for (int i = 0; i < D; ++i) K[i] = P[i][0] * rs;
    SS_UNROLL for (int i = 0; i < D; ++i) m[i] = fma(K[i], v, m[i]);
    SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = i; j < D; ++j) X[i][j] = X[j][i] = P[i][j] - K[i] * P[0][j] * 0.5 - K[j] * P[0][i] * 0.5; }
    SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) P[i][j] = X[i][j]; }
    *S = s;
    return -0.5 * (log(6.283185307179586476925 * s) + v * v * rs);
}

// ---- smoothing: element (E, g, L) over suffixes; the scan runs over r = N - 1 - k, so a (x) b has a the LATER step ------------------
template <int D> struct ss_smooth {
    static constexpr int NS = D * (D + 1) / 2, OE = 0, OG = D * D, OL = OG + D, NV = OL + NS;
    static constexpr int STATE = OG, NSTATE = D + NS;      // (g, L): the smoothed mean and covariance at the head of a suffix
    static SS_FN void identity(double (&v)[NV]) {
        SS_UNROLL for (int i = 0; i < NV; ++i) v[i] = 0.0;
        SS_UNROLL for (int i = 0; i < D; ++i) v[OE + i * D + i] = 1.0;
    }
    static SS_FN void op(const double (&a)[NV], const double (&b)[NV], double (&o)[NV]) {     // (E_b E_a, E_b g_a + g_b, E_b L_a E_b^T + L_b)
        double Ea[D][D], Eb[D][D], La[D][D], X[D][D], Y[D][D], g[D], u[D];
        ss_load<D>(a + OE, Ea), ss_load<D>(b + OE, Eb), ss_unpack<D>(a + OL, La);
        SS_UNROLL for (int i = 0; i < D; ++i) g[i] = a[OG + i];
        ss_mv<D>(Eb, g, u);
        SS_UNROLL for (int i = 0; i < D; ++i) o[OG + i] = u[i] + b[OG + i];
        ss_mm<D>(Eb, La, X);
        ss_mm_nt<D>(X, Eb, Y);
        double Lb[D][D];
        ss_unpack<D>(b + OL, Lb);
        SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) Y[i][j] += Lb[i][j]; }
        ss_pack<D>(Y, o + OL);
        ss_mm<D>(Eb, Ea, X);
        ss_store<D>(X, o + OE);
    }
    // step k from its filtered moments (m, P) and the transition (A, Q) to step k + 1; last: k = N - 1; same: t_{k+1} == t_k (the
    // two steps share one state: the identity element, whatever P is)
    static SS_FN void element(const double (&A)[D][D], const double (&Q)[D][D], bool last, bool same, const double (&m)[D], const double (&P)[D][D],
                              double (&v)[NV]) {
        if (same) { identity(v); return; }
        if (last) {
            SS_UNROLL for (int i = 0; i < D * D; ++i) v[OE + i] = 0.0;
            SS_UNROLL for (int i = 0; i < D; ++i) v[OG + i] = m[i];
            ss_pack<D>(P, v + OL);
            return;
        }
        double G[D][D], Pp[D][D], X[D][D], Em[D][D], am[D], u[D];
        ss_mm<D>(A, P, G);                                     // G = A P
        ss_mm_nt<D>(G, A, X);
        SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) Pp[i][j] = 0.5 * (X[i][j] + X[j][i]) + Q[i][j]; }
        ss_spd_solve<D>(Pp, G, X);                             // E^T = (P^-)^-1 A P
        SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) Em[i][j] = X[j][i]; }
        ss_store<D>(Em, v + OE);
        ss_mv<D>(A, m, am);
        ss_mv<D>(Em, am, u);
        SS_UNROLL for (int i = 0; i < D; ++i) v[OG + i] = m[i] - u[i];       // g = m - E A m
        ss_mm<D>(Em, G, X);
        SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) X[i][j] = P[i][j] - X[i][j]; }
        ss_pack<D>(X, v + OL);                                 // L = P - E A P
    }
};

// ---- LML gradient: the sensitivity of the filter --------------------------------------------------------------------------------------
// d/dlambda of Pinf, A(dt) and Q(dt); A: ss_amat's.  dA = -dt A + e^(-x) d(polynomial part)/dlambda, with the two terms merged so that
// small x cancels nothing; dQ = dPinf - dA Pinf A^T - A dPinf A^T - A Pinf dA^T, symmetrised as ss_trans does
SS_FN void ss_dpinf(const ss_par &p, double (&P)[2][2]) { P[0][0] = P[0][1] = P[1][0] = 0.0, P[1][1] = 2.0 * p.lam * p.sf2; }
SS_FN void ss_dpinf(const ss_par &p, double (&P)[3][3]) {
    const double dk = 2.0 * p.lam / 3.0 * p.sf2;
    P[0][0] = P[0][1] = P[1][0] = P[1][2] = P[2][1] = 0.0, P[0][2] = P[2][0] = -dk, P[1][1] = dk, P[2][2] = 4.0 * p.lam * p.lam * p.lam * p.sf2;
}
SS_FN void ss_damat(const ss_par &p, double dt, double (&A)[2][2]) {
    const double x = p.lam * dt, e = exp(-x);
    A[0][0] = -e * x * dt, A[0][1] = -e * dt * dt, A[1][0] = e * x * (x - 2.0), A[1][1] = e * dt * (x - 2.0);
}
SS_FN void ss_damat(const ss_par &p, double dt, double (&A)[3][3]) {
    const double l = p.lam, x = l * dt, e = exp(-x), q = -0.5 * x * x + 3.0 * x - 3.0;
    A[0][0] = -e * 0.5 * dt * x * x, A[0][1] = -e * dt * dt * x, A[0][2] = -e * 0.5 * dt * dt * dt;
    A[1][0] = e * 0.5 * x * x * (x - 3.0), A[1][1] = e * dt * x * (x - 3.0), A[1][2] = e * 0.5 * dt * dt * (x - 3.0);
    A[2][0] = e * l * x * q, A[2][1] = e * 2.0 * x * q,A[2][2] = e * dt * q;
}
template <int D> SS_FN void ss_dtrans(const ss_par &p, double dt, bool first, const double (&A)[D][D], double (&dA)[D][D], double (&dQ)[D][D]) {
    double dPi[D][D];
    ss_dpinf(p, dPi);
    if (first) {
        SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) dA[i][j] = 0.0, dQ[i][j] = dPi[i][j]; }
        return;
    }
    double Pi[D][D], AP[D][D], Y[D][D], X[D][D], Z[D][D];
    ss_pinf(p, Pi);
    ss_damat(p, dt, dA);
    ss_mm<D>(A, Pi, AP);
    ss_mm_nt<D>(dA, AP, Y);                                    // dA Pinf A^T
    ss_mm<D>(A, dPi, X);
    ss_mm_nt<D>(X, A, Z);                                      // A dPinf A^T
    SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) dQ[i][j] = dPi[i][j] - (Y[i][j] + Y[j][i]) - 0.5 * (Z[i][j] + Z[j][i]); }
}

// What one observed step with transition (A, Q) from the filtered moments (m, P) of the step before shares between the directions:
// AP = A P, S = P^-_00 + R, rs = 1 / S, vs = v / S with v = y - (A m)_0, the gain K = P^- h / S
template <int D> struct ss_gain { double AP[D][D], K[D], S, rs, v, vs; };
template <int D> SS_FN void ss_make_gain(const double (&A)[D][D], const double (&Q)[D][D], const double (&m)[D], const double (&P)[D][D], double y, double R,
                                         ss_gain<D> &w) {
    double X[D][D], mp[D];
    ss_mm<D>(A, P, w.AP);
    ss_mm_nt<D>(w.AP, A, X);
    ss_mv<D>(A, m, mp);
    w.S = X[0][0] + Q[0][0] + R, w.rs = 1.0 / w.S, w.v = y - mp[0], w.vs = w.v * w.rs;
    SS_UNROLL for (int i = 0; i < D; ++i) w.K[i] = (0.5 * (X[i][0] + X[0][i]) + Q[i][0]) * w.rs;
}
// F = dA P A^T + A P dA^T + dQ
template <int D> SS_FN void ss_sens_forcing(const double (&dA)[D][D], const double (&dQ)[D][D], const ss_gain<D> &w, double (&F)[D][D]) {
    double X[D][D];
    ss_mm_nt<D>(dA, w.AP, X);
    SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) F[i][j] = X[i][j] + X[j][i] + dQ[i][j]; }
}
// u -> J u and M -> J M J^T + K K^T dR for J = I - K h^T, M symmetric
template <int D> SS_FN void ss_sens_project(const ss_gain<D> &w, double dR, double (&u)[D], double (&M)[D][D]) {
    double JM[D][D];
    const double u0 = u[0];
    SS_UNROLL for (int i = 0; i < D; ++i) u[i] -= w.K[i] * u0;
    SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) JM[i][j] = M[i][j] - w.K[i] * M[0][j]; }
    SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) M[i][j] = JM[i][j] - JM[i][0] * w.K[j] + w.K[i] * w.K[j] * dR; }
}

// The derivatives (dm, dP) of the filtered moments in a direction obey dP_k = Phi dP_{k-1} Phi^T + L, dm_k = Phi dm_{k-1} + Phi dP_{k-1} a + g
// with Phi = J A, a = A^T h v / S, L = J F J^T + K K^T dR, g = J (dA m + F h v / S) - K dR v / S: coefficients of the filter's trajectory
// alone, and no inverse.  The coupling of dm to dP keeps the form Phi X a under composition, and (Phi, a) do not depend on the direction,
// so ONE element carries both directions: (Phi, a, g_0, L_0, g_1, L_1), L packed.  Direction 0 is lambda (dA, dQ of ss_dtrans, dR = 0),
// direction 1 is R = sn^2 (dA = dQ = 0, dR = 1); the chain rule to (l, sn) is applied to the finished sums.  a (x) b with a the earlier.
// A prefix's (g_d, L_d) is (dm, dP) after its last step: all that a later step reads of it.
template <int D> struct ss_sens {
    static constexpr int NS = D * (D + 1) / 2, ND = 2, OP = 0, OA = D * D, OG = OA + D, NP = D + NS, NV = OG + ND * NP;
    static constexpr int STATE = OG, NSTATE = ND * NP;
    static SS_FN void identity(double (&v)[NV]) {
        SS_UNROLL for (int i = 0; i < NV; ++i) v[i] = 0.0;
        SS_UNROLL for (int i = 0; i < D; ++i) v[OP + i * D + i] = 1.0;
    }
    static SS_FN void op(const double (&x)[NV], const double (&z)[NV], double (&o)[NV]) {
        double Px[D][D], Pz[D][D], Lx[D][D], Lz[D][D], X[D][D], Y[D][D], az[D], u[D], w[D];
        ss_load<D>(x + OP, Px), ss_load<D>(z + OP, Pz);
        SS_UNROLL for (int i = 0; i < D; ++i) az[i] = z[OA + i];
        ss_mm<D>(Pz, Px, X);
        ss_store<D>(X, o + OP);                                // Phi = Phi_z Phi_x
        ss_mtv<D>(Px, az, u);
        SS_UNROLL for (int i = 0; i < D; ++i) o[OA + i] = x[OA + i] + u[i];   // a = a_x + Phi_x^T a_z
        SS_UNROLL for (int d = 0; d < ND; ++d) {
            const int og = OG + d * NP, ol = og + D;
            ss_unpack<D>(x + ol, Lx), ss_unpack<D>(z + ol, Lz);
            ss_mv<D>(Lx, az, u);
            SS_UNROLL for (int i = 0; i < D; ++i) u[i] += x[og + i];
            ss_mv<D>(Pz, u, w);
            SS_UNROLL for (int i = 0; i < D; ++i) o[og + i] = w[i] + z[og + i];          // g = Phi_z (g_x + L_x a_z) + g_z
            ss_mm<D>(Pz, Lx, X);
            ss_mm_nt<D>(X, Pz, Y);
            SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) Y[i][j] += Lz[i][j]; }
            ss_pack<D>(Y, o + ol);                             // L = Phi_z L_x Phi_z^T + L_z
        }
    }
    // the element of one observed step from its transition and its derivative and the gain at the filtered moments (m, P) before it
    static SS_FN void element(const double (&A)[D][D], const double (&dA)[D][D], const double (&dQ)[D][D], const double (&m)[D], const ss_gain<D> &w,
                              double (&v)[NV]) {
        double F[D][D], u[D];
        SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) v[OP + i * D + j] = A[i][j] - w.K[i] * A[0][j]; }
        SS_UNROLL for (int i = 0; i < D; ++i) v[OA + i] = A[0][i] * w.vs;
        ss_sens_forcing<D>(dA, dQ, w, F);
        ss_mv<D>(dA, m, u);
        SS_UNROLL for (int i = 0; i < D; ++i) u[i] = fma(F[i][0], w.vs, u[i]);
        ss_sens_project<D>(w, 0.0, u, F);
        SS_UNROLL for (int i = 0; i < D; ++i) v[OG + i] = u[i];
        ss_pack<D>(F, v + OG + D);
        SS_UNROLL for (int i = 0; i < D; ++i) v[OG + NP + i] = -w.K[i] * w.vs;
        SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = i; j < D; ++j) v[OG + NP + D + ss_sidx<D>(i, j)] = w.K[i] * w.K[j]; }
    }
};

// One step of the sensitivity recursion in both directions, beside ss_kalman_step and BEFORE it (m, P: the filtered moments of the step
// before): (dm, dP)[d] -> those of this step; dl[d] += the derivative of the step's LML term,
//     -1/2 dS (1/S - v^2/S^2) + v (dA m + A dm)_0 / S,   dS = (A dP A^T + F)_00 + dR
template <int D> SS_FN void ss_sens_step(const double (&A)[D][D], const double (&dA)[D][D], const double (&dQ)[D][D], const double (&m)[D],
                                         const ss_gain<D> &w, double (&dm)[2][D], double (&dP)[2][D][D], double (&dl)[2]) {
    double F[D][D], X[D][D], Y[D][D], u[D], dam[D];
    ss_sens_forcing<D>(dA, dQ, w, F);
    ss_mv<D>(dA, m, dam);
    SS_UNROLL for (int d = 0; d < 2; ++d) {
        const double dR = d == 0 ? 0.0 : 1.0;
        ss_mv<D>(A, dm[d], u);
        ss_mm<D>(A, dP[d], X);
        ss_mm_nt<D>(X, A, Y);
        SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = i; j < D; ++j) X[i][j] = X[j][i] = 0.5 * (Y[i][j] + Y[j][i]) + (d == 0 ? F[i][j] : 0.0); }
        if (d == 0) { SS_UNROLL for (int i = 0; i < D; ++i) u[i] += dam[i]; }
        dl[d] += fma(-0.5 * (X[0][0] + dR), w.rs - w.vs * w.vs, w.vs * u[0]);
        SS_UNROLL for (int i = 0; i < D; ++i) u[i] = fma(X[i][0], w.vs, u[i]);
        ss_sens_project<D>(w, dR, u, X);
        SS_UNROLL for (int i = 0; i < D; ++i) dm[d][i] = u[i] - dR * w.K[i] * w.vs;
        SS_UNROLL for (int i = 0; i < D; ++i) { SS_UNROLL for (int j = 0; j < D; ++j) dP[d][i][j] = X[i][j]; }
    }
}
