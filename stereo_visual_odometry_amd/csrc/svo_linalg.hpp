// svo_linalg.hpp — small dense f64 linear algebra for the geometry kernels (device code).
// One-sided Jacobi SVD (Hestenes) on REGISTER arrays of fixed compile-time sizes: every row and pair index is a compile-time
// constant, only the sweep loop is dynamic.  (Run-time indices would turn every access of a private array into a select chain or a
// scratch access.)  Each rule of the algorithm is stated once here — the pair step (hestenes_*), the descending sort (sort_desc)
// — and the 12 x 12 sweep of EPnP in svo_kernels_pnp.hip, which rotates rows in LDS, calls the same pieces.
// Only + - * / sqrt in a fixed order and no FMA contraction (-ffp-contract=off), so results are IEEE-reproducible.
#pragma once
#include <hip/hip_runtime.h>

#define SVO_DBL_EPS 2.2204460492503131e-16
#define SVO_DBL_MIN 2.2250738585072014e-308

// c and s of one Hestenes rotation (OpenCV's JacobiSVDImpl_): two arithmetically different forms, chosen by the sign of beta.
// The lanes of a wave disagree about that sign, so written as if / else the wave walks BOTH division -> square root -> division
// chains one after the other (~90 dependent f64 instructions instead of ~45).  Here the two forms share one instruction stream:
// the same operations on selected operands, the same bits.
__device__ __forceinline__ void jacobi_cs(double p, double beta, double gamma, double& c, double& s) {
    const bool neg = beta < 0;
    const double num = neg ? (gamma - beta) * 0.5 : gamma + beta;
    const double den = neg ? gamma : gamma * 2;
    const double r = sqrt(num / den);
    const double o = p / (gamma * r * 2);
    c = neg ? o : r;
    s = neg ? r : o;
}

// ---- one Hestenes pair step (the body of JacobiSVDImpl_'s pair loop) on rows x, y of length M with squared norms a, b ----
// a pair whose inner product p has |p| <= hestenes_limit(a, b) counts as orthogonal and is left alone
__device__ __forceinline__ double hestenes_limit(double a, double b) { return SVO_DBL_EPS * 10 * sqrt(a * b); }
__device__ __forceinline__ void hestenes_cs(double a, double b, double p, double& c, double& s) {
    p *= 2;
    const double beta = a - b, gamma = sqrt(p * p + beta * beta);
    jacobi_cs(p, beta, gamma, c, s);
}
// (x, y) <- (c x + s y, -s x + c y); a, b <- the squared norms of the rotated rows, summed in element order
template <int M>
__device__ __forceinline__ void hestenes_rotate(double* x, double* y, double c, double s, double& a, double& b) {
    a = b = 0;
#pragma unroll
    for (int k = 0; k < M; k++) {
        const double t0 = c * x[k] + s * y[k];
        const double t1 = -s * x[k] + c * y[k];
        x[k] = t0; y[k] = t1;
        a += t0 * t0; b += t1 * t1;
    }
}
// the whole step; false: the pair was not rotated (then c, s are not set)
template <int M>
__device__ __forceinline__ bool hestenes_pair(double* x, double* y, double& a, double& b, double& c, double& s) {
    double p = 0;
#pragma unroll
    for (int k = 0; k < M; k++) p += x[k] * y[k];
    if (fabs(p) <= hestenes_limit(a, b)) return false;
    hestenes_cs(a, b, p, c, s);
    hestenes_rotate<M>(x, y, c, s, a, b);
    return true;
}

// The descending selection sort that ends JacobiSVDImpl_ (the FIRST maximum wins ties), replayed with predicated moves: place i
// takes the first maximum of w[i ..], found at run time at place j, and swap(i, k, k == j) is called for every k > i so that
// whatever belongs to the values (rows, indices) travels with them.
template <int N, typename Swap>
__device__ __forceinline__ void sort_desc(double (&w)[N], Swap swap) {
#pragma unroll
    for (int i = 0; i < N - 1; i++) {
        int j = i; double wj = w[i];
#pragma unroll
        for (int k = i + 1; k < N; k++) { const bool g = wj < w[k]; j = g ? k : j; wj = g ? w[k] : wj; }
#pragma unroll
        for (int k = i + 1; k < N; k++) {
            const bool e = j == k;
            { const double x = w[i], y = w[k]; w[i] = e ? y : x; w[k] = e ? x : y; }
            swap(i, k, e);
        }
    }
}
// ... on (value, index) pairs: perm[i] = the place the value now at i started from
template <int N>
__device__ __forceinline__ void sort_desc_perm(double (&w)[N], int (&perm)[N]) {
#pragma unroll
    for (int i = 0; i < N; i++) perm[i] = i;
    sort_desc<N>(w, [&](int i, int k, bool e) { const int x = perm[i], y = perm[k]; perm[i] = e ? y : x; perm[k] = e ? x : y; });
}

// The sweeps.  At: N rows of length M (the transpose of an M x N matrix, M >= N).  On exit the rows of At are the left singular
// vectors times their singular values, Wv the singular values and the rows of Vt the right singular vectors — all UNSORTED.
template <int M, int N>
__device__ __forceinline__ void jacobi_sweeps(double (&At)[N][M], double (&Wv)[N], double (&Vt)[N][N]) {
    constexpr int max_iter = M > 30 ? M : 30;
#pragma unroll
    for (int i = 0; i < N; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < M; k++) sd += At[i][k] * At[i][k];
        Wv[i] = sd;
#pragma unroll
        for (int k = 0; k < N; k++) Vt[i][k] = i == k ? 1.0 : 0.0;
    }
#pragma unroll 1
    for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
#pragma unroll
        for (int i = 0; i < N - 1; i++) {
#pragma unroll
            for (int j = i + 1; j < N; j++) {
                double c, s, va, vb;
                if (!hestenes_pair<M>(At[i], At[j], Wv[i], Wv[j], c, s)) continue;
                changed = true;
                hestenes_rotate<N>(Vt[i], Vt[j], c, s, va, vb);        // (the norms of V's rows are not needed)
            }
        }
        if (!changed) break;
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < M; k++) sd += At[i][k] * At[i][k];
        Wv[i] = sqrt(sd);
    }
}

// The full decomposition: singular values descending, rows of At the left singular vectors (normalised if asked), rows of Vt the
// right ones.  Everything is inlined, so a caller pays only for the outputs it reads.
template <int M, int N>
__device__ __forceinline__ void jacobi_svd_reg(double (&At)[N][M], double (&Wv)[N], double (&Vt)[N][N], bool normalize) {
    const double minval = SVO_DBL_MIN;
    jacobi_sweeps<M, N>(At, Wv, Vt);
    sort_desc<N>(Wv, [&](int i, int k, bool e) {
#pragma unroll
        for (int c = 0; c < M; c++) { const double x = At[i][c], y = At[k][c]; At[i][c] = e ? y : x; At[k][c] = e ? x : y; }
#pragma unroll
        for (int c = 0; c < N; c++) { const double x = Vt[i][c], y = Vt[k][c]; Vt[i][c] = e ? y : x; Vt[k][c] = e ? x : y; }
    });
    if (normalize) {
#pragma unroll
        for (int i = 0; i < N; i++) {
            const double sd = Wv[i];
            const double s = sd > minval ? 1 / sd : 0.;
#pragma unroll
            for (int k = 0; k < M; k++) At[i][k] *= s;
        }
    }
}

// The right singular vector of the SMALLEST singular value of a row-major 4 x 4 matrix (the null vector of the triangulation's DLT
// system): the last row of Vt.  The left singular vectors are not read, so their part of the sort costs nothing.
__device__ inline void svd4_null_vector(const double (&A)[4][4], double (&X)[4]) {
    double At[4][4], Vt[4][4], Wv[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
#pragma unroll
        for (int j = 0; j < 4; j++) At[i][j] = A[j][i];
    }
    jacobi_svd_reg<4, 4>(At, Wv, Vt, false);
#pragma unroll
    for (int c = 0; c < 4; c++) X[c] = Vt[3][c];
}

// SVD of a row-major M x N matrix A.  Ut: N x M, Vt: N x N.
template <int M, int N>
__device__ void svd_rm(const double* A, double* Wv, double* Ut, double* Vt) {
    double At[N][M], W[N], V[N][N];
#pragma unroll
    for (int i = 0; i < N; i++) {
#pragma unroll
        for (int j = 0; j < M; j++) At[i][j] = A[j * N + i];
    }
    jacobi_svd_reg<M, N>(At, W, V, true);
#pragma unroll
    for (int i = 0; i < N; i++) {
        Wv[i] = W[i];
#pragma unroll
        for (int j = 0; j < M; j++) Ut[i * M + j] = At[i][j];
#pragma unroll
        for (int j = 0; j < N; j++) Vt[i * N + j] = V[i][j];
    }
}

// x = pinv(A) b for A: 6 x n (n = 3, 4, 5) on REGISTERS.  The three beta approximations of EPnP solve 6x4, 6x3 and 6x5 systems on
// three lanes of one wave — as three template instances they were three code paths the wave executed one after the other; here
// the system is zero-padded to five columns so that they run one instruction stream.  A zero row of At never rotates (p = 0 <= eps sqrt(a b) = 0), keeps its singular
// value 0 (<= the threshold: dropped) and leaves the identity columns of Vt alone, so the n x n part is computed exactly as the
// unpadded routine computes it, bit for bit.
__device__ inline void svd_solve6_reg(const double* A, int n, const double* b, double* x) {
    constexpr int M = 6, N = 5;
    double At[N][M], Wv[N], Vt[N][N];
#pragma unroll
    for (int i = 0; i < N; i++) {
#pragma unroll
        for (int j = 0; j < M; j++) At[i][j] = i < n ? A[j * n + i] : 0.0;
    }
    jacobi_svd_reg<M, N>(At, Wv, Vt, true);
    double thr = 0;
#pragma unroll
    for (int i = 0; i < N; i++) thr += Wv[i];
    thr *= SVO_DBL_EPS * 2;
    double xx[N] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < N; i++) {
        if (Wv[i] <= thr) continue;
        double s = 0;
#pragma unroll
        for (int k = 0; k < M; k++) s += At[i][k] * b[k];
        s /= Wv[i];
#pragma unroll
        for (int k = 0; k < N; k++) xx[k] += s * Vt[i][k];
    }
#pragma unroll
    for (int k = 0; k < N; k++) if (k < n) x[k] = xx[k];
}

__device__ inline void inv3_svd(const double A[9], double Ainv[9]) {
    double Wv[3], Ut[9], Vt[9];
    svd_rm<3, 3>(A, Wv, Ut, Vt);
    double thr = (Wv[0] + Wv[1] + Wv[2]) * SVO_DBL_EPS * 2;
    for (int i = 0; i < 9; i++) Ainv[i] = 0;
    for (int k = 0; k < 3; k++) {
        if (Wv[k] <= thr) continue;
        double iw = 1 / Wv[k];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Ainv[i * 3 + j] += Vt[k * 3 + i] * iw * Ut[k * 3 + j];
    }
}

// Householder QR least squares for the 6 x 4 Gauss-Newton step of EPnP, on registers with compile-time indices: A (destroyed),
// b (destroyed) -> x.  false if singular.
__device__ __forceinline__ bool qr_solve64_reg(double (&A)[6][4], double (&b)[6], double (&x)[4]) {
    constexpr int M = 6, N = 4;
    double A1[N], A2[N];
#pragma unroll
    for (int k = 0; k < N; k++) {
        double eta = 0;
#pragma unroll
        for (int i = k; i < M; i++) { double e = fabs(A[i][k]); if (eta < e) eta = e; }
        if (eta == 0) return false;
        double sum2 = 0, inv_eta = 1. / eta;
#pragma unroll
        for (int i = k; i < M; i++) { A[i][k] *= inv_eta; sum2 += A[i][k] * A[i][k]; }
        double sigma = sqrt(sum2);
        if (A[k][k] < 0) sigma = -sigma;
        A[k][k] += sigma;
        A1[k] = sigma * A[k][k];
        A2[k] = -eta * sigma;
#pragma unroll
        for (int j = k + 1; j < N; j++) {
            double sum = 0;
#pragma unroll
            for (int i = k; i < M; i++) sum += A[i][k] * A[i][j];
            double tau = sum / A1[k];
#pragma unroll
            for (int i = k; i < M; i++) A[i][j] -= tau * A[i][k];
        }
    }
#pragma unroll
    for (int j = 0; j < N; j++) {
        double tau = 0;
#pragma unroll
        for (int i = j; i < M; i++) tau += A[i][j] * b[i];
        tau /= A1[j];
#pragma unroll
        for (int i = j; i < M; i++) b[i] -= tau * A[i][j];
    }
    x[N - 1] = b[N - 1] / A2[N - 1];
#pragma unroll
    for (int i = N - 2; i >= 0; i--) {
        double sum = 0;
#pragma unroll
        for (int j = i + 1; j < N; j++) sum += A[i][j] * x[j];
        x[i] = (b[i] - sum) / A2[i];
    }
    return true;
}

// Rodrigues: rotation vector -> matrix (+ optional 3x9 Jacobian dR/dr), and matrix -> vector.
__device__ inline void rodrigues_to_matrix(const double r[3], double R[9], double* J) {
    double theta = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (theta < SVO_DBL_EPS) {
        for (int i = 0; i < 9; i++) R[i] = 0;
        R[0] = R[4] = R[8] = 1;
        if (J) { for (int i = 0; i < 27; i++) J[i] = 0; J[5] = J[15] = J[19] = -1; J[7] = J[11] = J[21] = 1; }
        return;
    }
    double c, s;
    sincos(theta, &s, &c);                                             // one argument reduction for both
    double c1 = 1. - c, itheta = 1. / theta;
    double rx = r[0] * itheta, ry = r[1] * itheta, rz = r[2] * itheta;
    double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = c * I[k] + c1 * rrt[k] + s * r_x[k];
    if (J) {
        double drrt[27] = {rx + rx, ry, rz, ry, 0, 0, rz, 0, 0,
                           0, rx, 0, rx, ry + ry, rz, 0, rz, 0,
                           0, 0, rx, 0, 0, ry, rx, ry, rz + rz};
        const double d_r_x_[27] = {0, 0, 0, 0, 0, -1, 0, 1, 0,
                                   0, 0, 1, 0, 0, 0, -1, 0, 0,
                                   0, -1, 0, 1, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 3; i++) {
            double ri = i == 0 ? rx : i == 1 ? ry : rz;
            double a0 = -s * ri, a1 = (s - 2 * c1 * itheta) * ri, a2 = c1 * itheta;
            double a3 = (c - s * itheta) * ri, a4 = s * itheta;
#pragma unroll
            for (int k = 0; k < 9; k++)
                J[i * 9 + k] = a0 * I[k] + a1 * rrt[k] + a2 * drrt[i * 9 + k] + a3 * r_x[k] + a4 * d_r_x_[i * 9 + k];
        }
    }
}

__device__ inline void rodrigues_to_vector(const double Rin[9], double r[3]) {
    double Wv[3], Ut[9], Vt[9], R[9];
    svd_rm<3, 3>(Rin, Wv, Ut, Vt);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += Ut[k * 3 + i] * Vt[k * 3 + j];
        R[i * 3 + j] = s;
    }
    double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
    double s = sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
    double c = (R[0] + R[4] + R[8] - 1) * 0.5;
    c = c > 1. ? 1. : c < -1. ? -1. : c;
    double theta = acos(c);
    if (s < 1e-5) {
        if (c > 0) { rx = ry = rz = 0; }
        else {
            double t;
            t = (R[0] + 1) * 0.5; rx = sqrt(t > 0. ? t : 0.);
            t = (R[4] + 1) * 0.5; ry = sqrt(t > 0. ? t : 0.) * (R[1] < 0 ? -1. : 1.);
            t = (R[8] + 1) * 0.5; rz = sqrt(t > 0. ? t : 0.) * (R[2] < 0 ? -1. : 1.);
            if (fabs(rx) < fabs(ry) && fabs(rx) < fabs(rz) && (R[5] > 0) != (ry * rz > 0)) rz = -rz;
            theta /= sqrt(rx * rx + ry * ry + rz * rz);
            rx *= theta; ry *= theta; rz *= theta;
        }
    } else {
        double vth = 1 / (2 * s);
        vth *= theta;
        rx *= vth; ry *= vth; rz *= vth;
    }
    r[0] = rx; r[1] = ry; r[2] = rz;
}
