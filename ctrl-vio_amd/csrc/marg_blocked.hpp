// marg_blocked.hpp -- prior construction on the device for windows beyond the in-LDS eigen-solver (marg_device.hpp, MARG_MAXD):
// m or n up to MARG_MAXD_BLOCKED.  Same algebra as k_marginalize (reference MarginalizationInfo::marginalize,
// marginalization_factor.cpp:189-265), one window at a time, each step a multi-workgroup launch over HBM scratch sized from m and n:
//
//   k_mb_gather   Amm (padded), [Amr | g_m] straight from HppS / WS / HllS / gS through the index lists (no dense N x N A)
//   block Jacobi  Amm = Vm diag(em) Vm^T          (mb_jacobi in ctvio.hip drives the three kernels below)
//   k_mb_y, k_mb_x X = Vm diag(1/em) Vm^T [Amr | g_m]   (eigenvalues <= eps dropped)
//   k_mb_reduce   A' = Arr - Amr^T X (symmetrised), b' = g_r - Amr^T x_b
//   block Jacobi  A' = V S V^T
//   k_mb_rank, k_mb_j0   J0 = sqrt(S) V^T, r0 = S^-1/2 V^T b', rows in ascending eigenvalue order (ties by index)
//
// BLOCK TWO-SIDED JACOBI.  The matrix (dimension nd) is padded to D = 64 * ceil(nd / 64) with decoupled zero rows and columns and
// split into D / 32 column blocks.  One sweep is a round-robin tournament over the blocks (rr_pair): per step, every block pair
// (p, q) is a 64 x 64 sub-problem; k_mb_pair loads it into LDS, runs one parallel cyclic Jacobi sweep on it (jacobi_core.hpp: the
// tournament, rotation rule and 2 x 2-block updates of jacobi_packed) and forms its rotation Q explicitly; k_mb_update then applies
// A <- Q^T A Q to every off-diagonal 64 x 64 tile of the step's pairs (one workgroup per tile: the tile depends only on itself and
// two Q, so the update is in place) and V <- V Q.  The diagonal tiles keep the rotated matrix of the LDS sweep.  A padded column meets
// only zero entries, so its rotations are the identity: it stays an exact zero eigenpair at its own index and is dropped.  After every
// sweep k_mb_mass sums the off-diagonal and diagonal mass per column block; the host adds the partials in block order and applies
// jacobi_converged (jacobi_core.hpp), as jacobi_packed does.  No floating-point atomics and no cross-workgroup synchronisation: equal
// inputs give equal bits.
#pragma once
#include "marg_device.hpp"

namespace ctv {

constexpr int MARG_MAXD_BLOCKED = 1024;   // largest m or n of the blocked path
constexpr int MB_BLK = 32;                // columns per block; a block pair is one 64 x 64 sub-problem
constexpr int MB_MAX_SWEEPS = 40;         // outer sweeps (the model, tests/marg_blocked_helpers.py: 2 for Amm, 14 for A' at m 268 / n 553)

__host__ __device__ inline int mb_padded(int nd) { return nd <= 64 ? 64 : (nd + 63) / 64 * 64; }

// one blocked window: sizes and device pointers into the scratch / outputs (passed by value)
struct MbWin {
  int32_t w, m, n, dm, dn;
  const int32_t *im, *ik;
  double *Bm, *Vm, *Bn, *Vn, *G, *Y, *X, *bp;   // Bm, Vm: dm x dm; Bn, Vn: dn x dn; G = [Amr | g_m], Y, X: m x (n + 1); b': n
  double *J0, *r0;
  int32_t *rank;
};

__global__ __launch_bounds__(256) void k_mb_gather(Dev d, MbWin b) {
  const WinMeta &wm = d.wins[b.w];
  const int cset = d.lm[b.w].cur;
  const double *g = d.gS[cset] + wm.u0;
  const long long stride = (long long)gridDim.x * blockDim.x, t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int m = b.m, n = b.n;
  for (long long e = t0; e < (long long)b.dm * b.dm; e += stride) {
    const int i = (int)(e / b.dm), j = (int)(e % b.dm);
    b.Bm[e] = (i < m && j < m) ? normal_eq_entry(d, wm, cset, b.im[i], b.im[j]) : 0.0;
    b.Vm[e] = (i == j) ? 1.0 : 0.0;
  }
  for (long long e = t0; e < (long long)m * (n + 1); e += stride) {
    const int i = (int)(e / (n + 1)), c = (int)(e % (n + 1));
    b.G[e] = c < n ? normal_eq_entry(d, wm, cset, b.im[i], b.ik[c]) : g[b.im[i]];
  }
  for (long long e = t0; e < (long long)b.dn * b.dn; e += stride) b.Vn[e] = (e / b.dn == e % b.dn) ? 1.0 : 0.0;
}

// ---- block two-sided Jacobi

// global index of local row / column l (0..63) of block pair i at tournament step s
__device__ __forceinline__ void mb_group(int nb, int s, int i, int &bp, int &bq) { rr_pair(nb, s, i, bp, bq); }
__device__ __forceinline__ int mb_gl(int bp, int bq, int l) { return l < MB_BLK ? bp * MB_BLK + l : bq * MB_BLK + l - MB_BLK; }

// per column block: sum of squares below the diagonal and on it (fixed thread mapping and tree: deterministic)
__global__ __launch_bounds__(256) void k_mb_mass(const double *B, int D, double *part) {
  __shared__ double red[512];
  const int tid = threadIdx.x, j = blockIdx.x * MB_BLK + (tid & (MB_BLK - 1));
  double off = 0.0, dia = 0.0;
  for (int i = j + 1 + (tid >> 5); i < D; i += 256 / MB_BLK) { const double v = B[(long long)i * D + j]; off += v * v; }
  if (tid < MB_BLK) { const double v = B[(long long)j * D + j]; dia = v * v; }
  red[tid] = off; red[256 + tid] = dia;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) { if (tid < st) { red[tid] += red[tid + st]; red[256 + tid] += red[256 + tid + st]; } __syncthreads(); }
  if (tid == 0) { part[2 * blockIdx.x] = red[0]; part[2 * blockIdx.x + 1] = red[256]; }
}

// one workgroup per block pair of step s: one parallel cyclic Jacobi sweep on the 64 x 64 sub-problem in LDS (packed lower triangle,
// one sweep of jacobi_packed without its dummy player), Q accumulated explicitly; the rotated sub-problem goes back to B, Q to Qs
__global__ __launch_bounds__(256) void k_mb_pair(double *B, int D, int s, double *Qs) {
  constexpr int W = 2 * MB_BLK, NPK = W * (W + 1) / 2, HALF = W / 2, NBLK = HALF * (HALF + 1) / 2;
  __shared__ double Apk[NPK];
  __shared__ double Q[W * W];
  __shared__ double cs[W];
  __shared__ int pq[W];
  const int tid = threadIdx.x;
  int bp, bq;
  mb_group(D / MB_BLK, s, blockIdx.x, bp, bq);
  for (int e = tid; e < NPK; e += 256) {
    int i, j;
    tri_decode(e, i, j);
    Apk[e] = B[(long long)mb_gl(bp, bq, i) * D + mb_gl(bp, bq, j)];
  }
  for (int e = tid; e < W * W; e += 256) Q[e] = (e / W == e % W) ? 1.0 : 0.0;
  __syncthreads();
  for (int st = 0; st < W - 1; ++st) {
    if (tid < HALF) {
      int p, q;
      rr_pair(W, st, tid, p, q);
      double c, sn;
      jacobi_cs(Apk, p, q, c, sn);
      cs[2 * tid] = c; cs[2 * tid + 1] = sn; pq[2 * tid] = p; pq[2 * tid + 1] = q;
    }
    __syncthreads();
    for (int e = tid; e < NBLK; e += 256) {
      int I, J;
      tri_decode(e, I, J);
      const int p1 = pq[2 * I], q1 = pq[2 * I + 1], p2 = pq[2 * J], q2 = pq[2 * J + 1];
      const double c1 = cs[2 * I], s1 = cs[2 * I + 1], c2 = cs[2 * J], s2 = cs[2 * J + 1];
      if (I != J) jacobi_block_update<false>(Apk, W, p1, q1, p2, q2, c1, s1, c2, s2);
      else jacobi_diag_update(Apk, p1, q1, c1, s1);
    }
    for (int e = tid; e < W * HALF; e += 256) {   // Q <- Q R (columns p, q of every row)
      const int row = e / HALF, i = e % HALF;
      rotate_cols(Q, row * W + pq[2 * i], row * W + pq[2 * i + 1], cs[2 * i], cs[2 * i + 1]);
    }
    __syncthreads();
  }
  for (int e = tid; e < W * W; e += 256) {
    const int i = e / W, j = e % W;
    B[(long long)mb_gl(bp, bq, i) * D + mb_gl(bp, bq, j)] = Apk[pk_idx(i, j)];
    Qs[(size_t)blockIdx.x * W * W + e] = Q[e];
  }
}

// the two-sided update of step s.  Workgroups [0, npair (npair - 1) / 2): off-diagonal tile (k, l), k > l, of the step's block pairs:
// T <- Q_k^T T Q_l, written to (k, l) and, transposed, to (l, k) -- B stays exactly symmetric.  The rest: rows [64 rt, 64 rt + 64) of V,
// columns of pair k: T <- T Q_k.  Every workgroup reads and writes only its own tile(s): in place.
__global__ __launch_bounds__(256) void k_mb_update(double *B, double *V, int D, int s, const double *Qs) {
  constexpr int W = 2 * MB_BLK;
  __shared__ double T[W * W];
  const int tid = threadIdx.x, nb = D / MB_BLK, npair = nb / 2, noff = npair * (npair - 1) / 2;
  int it = blockIdx.x;
  int rp = -1, rq = -1, cp, cq, rt = 0;
  double *M;
  const double *Ql, *Qr = nullptr;
  if (it < noff) {
    int k, l;
    tri_decode_strict(it, k, l);
    mb_group(nb, s, k, rp, rq);
    mb_group(nb, s, l, cp, cq);
    M = B; Qr = Qs + (size_t)k * W * W; Ql = Qs + (size_t)l * W * W;
  } else {
    it -= noff;
    rt = it / npair;
    const int k = it % npair;
    mb_group(nb, s, k, cp, cq);
    M = V; Ql = Qs + (size_t)k * W * W;
  }
  auto row_of = [&](int r) { return rp >= 0 ? mb_gl(rp, rq, r) : rt * W + r; };
  for (int e = tid; e < W * W; e += 256) T[e] = M[(long long)row_of(e / W) * D + mb_gl(cp, cq, e % W)];
  __syncthreads();
  const int c = tid & (W - 1), r0 = (tid >> 6) * 16;
  double acc[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0;
  for (int k = 0; k < W; ++k) {
    const double q = Ql[k * W + c];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = fma(T[(r0 + r) * W + k], q, acc[r]);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) T[(r0 + r) * W + c] = acc[r];
  __syncthreads();
  if (!Qr) {
#pragma unroll
    for (int r = 0; r < 16; ++r) M[(long long)row_of(r0 + r) * D + mb_gl(cp, cq, c)] = acc[r];
    return;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0;
  for (int k = 0; k < W; ++k) {
    const double u = T[k * W + c];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = fma(Qr[k * W + r0 + r], u, acc[r]);
  }
  const int gc = mb_gl(cp, cq, c);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int gr = row_of(r0 + r);
    M[(long long)gr * D + gc] = acc[r];
    M[(long long)gc * D + gr] = acc[r];
  }
}

// ---- elimination: Y = diag(1 / em) Vm^T [Amr | g_m] (eigenvalues <= eps dropped), X = Vm Y
__global__ __launch_bounds__(256) void k_mb_y(MbWin b, double eps) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int n1 = b.n + 1;
  if (e >= (long long)b.m * n1) return;
  const int a = (int)(e / n1), c = (int)(e % n1);
  const double ev = b.Bm[(long long)a * b.dm + a];
  double s = 0.0;
  if (ev > eps) {
    for (int i = 0; i < b.m; ++i) s += b.Vm[(long long)i * b.dm + a] * b.G[(long long)i * n1 + c];
    s /= ev;
  }
  b.Y[e] = s;
}

__global__ __launch_bounds__(256) void k_mb_x(MbWin b) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int n1 = b.n + 1;
  if (e >= (long long)b.m * n1) return;
  const int i = (int)(e / n1), c = (int)(e % n1);
  double s = 0.0;
  for (int a = 0; a < b.m; ++a) s += b.Vm[(long long)i * b.dm + a] * b.Y[(long long)a * n1 + c];
  b.X[e] = s;
}

// A' = Arr - Amr^T X (symmetrised; zero padding to dn x dn) and b' = g_r - Amr^T x_b
__global__ __launch_bounds__(256) void k_mb_reduce(Dev d, MbWin b) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int n = b.n, n1 = n + 1, dn = b.dn;
  const WinMeta &wm = d.wins[b.w];
  const int cset = d.lm[b.w].cur;
  if (e < (long long)dn * dn) {
    const int r = (int)(e / dn), c = (int)(e % dn);
    double v = 0.0;
    if (r < n && c < n) {
      double s1 = normal_eq_entry(d, wm, cset, b.ik[r], b.ik[c]), s2 = normal_eq_entry(d, wm, cset, b.ik[c], b.ik[r]);
      for (int i = 0; i < b.m; ++i) {
        s1 -= b.G[(long long)i * n1 + r] * b.X[(long long)i * n1 + c];
        s2 -= b.G[(long long)i * n1 + c] * b.X[(long long)i * n1 + r];
      }
      v = 0.5 * (s1 + s2);
    }
    b.Bn[e] = v;
  } else if (e < (long long)dn * dn + n) {
    const int r = (int)(e - (long long)dn * dn);
    double s = d.gS[cset][wm.u0 + b.ik[r]];
    for (int i = 0; i < b.m; ++i) s -= b.G[(long long)i * n1 + r] * b.X[(long long)i * n1 + n];
    b.bp[r] = s;
  }
}

// ---- factor: rank of every eigenvalue (ascending, ties by index) and r0[rank a] = S_a^-1/2 V[:, a]^T b'
__global__ __launch_bounds__(256) void k_mb_rank(MbWin b, double eps) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= b.n) return;
  const long long dn = b.dn;
  const double ea = b.Bn[a * dn + a];
  int rk = 0;
  for (int k = 0; k < b.n; ++k) {
    const double ek = b.Bn[k * dn + k];
    rk += (ek < ea || (ek == ea && k < a)) ? 1 : 0;
  }
  b.rank[a] = rk;
  double s = 0.0;
  for (int i = 0; i < b.n; ++i) s += b.Vn[i * dn + a] * b.bp[i];
  const double S = ea > eps ? ea : 0.0;
  b.r0[rk] = S > 0.0 ? s / sqrt(S) : 0.0;
}

// J0[rank a][i] = sqrt(S_a) V[i][a]
__global__ __launch_bounds__(256) void k_mb_j0(MbWin b, double eps) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)b.n * b.n) return;
  const int i = (int)(e / b.n), a = (int)(e % b.n);
  const long long dn = b.dn;
  const double ea = b.Bn[a * dn + a];
  const double S = ea > eps ? ea : 0.0;
  b.J0[(long long)b.rank[a] * b.n + i] = sqrt(S) * b.Vn[i * dn + a];
}

}  // namespace ctv
