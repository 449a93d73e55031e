// k_batch_simplex: the loop of LPSolver.simplex (LPSolver.java:101-107) for MANY SMALL LPs in one launch.
// Included from lpx_kernels.hip inside lpxk::plain / lpxk::fused like every other arithmetic kernel.
//
// One workgroup per LP.  The workgroup pulls its LP's image (BatchLayout, lpx_kernels.h: A with an odd row pitch, b, c, v,
// perm) from HBM into LDS with 16-byte accesses, runs the whole loop on chip and stores the image back, so a later launch
// resumes from it.  Nothing is shared between workgroups: no persistent grid, no spinning, the hardware hands the
// workgroups out as CUs come free.
//
// One iteration, in the order of the reference's loop (entering or OPTIMAL; leaving or UNBOUNDED; budget; tracked slot;
// pivot; count), costs three workgroup barriers:
//   leaving    thread i takes rows i, i+T, ...: saves A[i][e] into col[i] (the entering column, before anything is
//              overwritten) and folds ratio_of(A[i][e], b[i]) into the lexicographic minimum on (ratio, row), a NaN or
//              a ratio not below 1e50 never entering it (k_ratio_gather's rule)                               -- barrier L
//   row l      thread j takes columns j, j+T, ...: prow[j] /= piv (prow[e] = 1/piv), c[j] = submul(c[j], pc, prow[j])
//              (c[e] = -(pc/piv)), and folds the NEW c[j] into the next iteration's entering choice            -- barrier B1
//   the rest   column e and b row-parallel (A[i][e] = -(col[i]/piv), b[i] = submul(b[i], col[i], b[l]));  every other
//              entry by 64-column chunks: a wave holds prow[j] of its chunk in a register and walks down the rows of its
//              row group, the multiplier col[i] being a broadcast read and A[i][j] contiguous across the lanes;
//              thread 0 meanwhile writes b[l], v = addmul(v, b[l], pc) and swaps perm[e] with perm[n+l]      -- barrier B2
// Every entry sees the reference's operations in the reference's order (lp_oracle.hpp:200-233); which thread performs
// them changes no bit.  A zero multiplier is never skipped.  Waves of a workgroup: NW = T/64; with NQ = ceil(n/64) column
// chunks there are G = max(1, NW/NQ) row groups and wave w takes the units u = w, w+NW, ... < NQ*G (chunk u % NQ, rows
// u / NQ, u / NQ + G, ...).  A one-wave workgroup (T = 64) compiles without barrier instructions.

// (key, slot) of the entering choice as a RatioRow so that one lexicographic minimum serves both rules: the reference's
// (first slot with c[j] > 1e-9: key 0) and Dantzig's (largest c[j], lowest slot on ties: key -c[j]).
__device__ __forceinline__ void batch_consider(RatioRow& best, double cj, int j, int dantzig) {
  if (cj > kEps) best = rr_min(best, RatioRow{dantzig ? -cj : 0.0, j, 0});
}

// workgroup-wide lexicographic minimum with ONE barrier; `sh` (16 entries) must not be in use by another reduction
__device__ __forceinline__ RatioRow batch_reduce(RatioRow x, RatioRow* sh, int lane, int wave, int nw) {
  x = rr_wave_min(x);
  if (lane == 0) sh[wave] = x;
  __syncthreads();
  RatioRow r = sh[0];
  for (int w = 1; w < nw; ++w) r = rr_min(r, sh[w]);
  return r;
}

template <int kThreads>
__global__ __launch_bounds__(kThreads) void k_batch_simplex(const BatchArgs a) {
  extern __shared__ __attribute__((aligned(16))) double batch_lds[];
  const int k = blockIdx.x;
  if (k >= a.count) return;
  const int m = a.m[k], n = a.n[k];
  const BatchLayout L = batch_layout(m, n);
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = T >> 6;
  if (L.lds_bytes > a.lds_bytes) {  // the host sized the launch from the same formula: never taken, and never out of bounds
    if (tid == 0) { a.status[k] = 7 /* LPX_DEVICE_ERROR */; a.pivots[k] = 0; }
    return;
  }
  double* const image = a.image + a.offset[k];
  const int nvec = (int)(L.image >> 1);
  for (int q = tid; q < nvec; q += T) ((d2*)batch_lds)[q] = ((const d2*)image)[q];

  const int ld = (int)L.ld;
  double* const A = batch_lds;
  double* const b = batch_lds + L.b;
  double* const c = batch_lds + L.c;
  double* const vp = batch_lds + L.v;
  int32_t* const perm = (int32_t*)(batch_lds + L.perm);
  double* const col = batch_lds + L.col;
  RatioRow* const sh_e = (RatioRow*)(col + ((m + 1) & ~1));
  RatioRow* const sh_l = sh_e + 16;
  const int dantzig = a.dantzig;
  const int nq = (n + 63) >> 6;
  const int groups = nq > 0 && nw > nq ? nw / nq : 1;
  __syncthreads();

  int64_t pivots = 0;
  int track = a.track[k];
  int status;
  RatioRow ent = rr_none();
  for (int j = tid; j < n; j += T) batch_consider(ent, c[j], j, dantzig);
  ent = batch_reduce(ent, sh_e, lane, wave, nw);
  for (;;) {
    const int e = ent.row == INT_MAX ? -1 : ent.row;                                // :101
    if (e < 0) { status = 0 /* LPX_OPTIMAL */; break; }
    RatioRow best = rr_none();                                                      // getLeaving, LPState.java:287-305
    for (int i = tid; i < m; i += T) {
      const double aie = A[i * ld + e];
      col[i] = aie;
      const double r = ratio_of(aie, b[i]);
      if (r < kInf) best = rr_min(best, RatioRow{r, i, 0});
    }
    best = batch_reduce(best, sh_l, lane, wave, nw);                                // barrier L
    if (!(best.ratio < kInf)) { status = 1 /* LPX_UNBOUNDED */; break; }            // :103-106
    if (a.max_pivots >= 0 && pivots >= a.max_pivots) { status = 9 /* LPX_PIVOT_LIMIT */; break; }
    const int l = best.row;
    if (track >= 0) {                                                               // LPSolver.java:151-155
      if (e == track) track = l + n;
      else if (l + n == track) track = e;
    }
    // pivot(e, l), LPState.java:133-181.  piv, pc and b[l] are read here by every thread; their new values are stored
    // behind barrier B1 only
    const double piv = col[l], pc = c[e];
    const double bl = __ddiv_rn(b[l], piv);                                         // :146
    double* const prow = A + l * ld;
    double ce_new = 0.0;
    ent = rr_none();
    for (int j = tid; j < n; j += T) {
      if (j == e) {
        prow[j] = __ddiv_rn(1.0, piv);                                              // :139
        ce_new = -__ddiv_rn(pc, piv);                                               // :172
        batch_consider(ent, ce_new, j, dantzig);
      } else {
        const double pr = __ddiv_rn(prow[j], piv);                                  // :144
        const double cn = submul(c[j], pc, pr);                                     // :177
        prow[j] = pr;
        c[j] = cn;
        batch_consider(ent, cn, j, dantzig);
      }
    }
    ent = batch_reduce(ent, sh_e, lane, wave, nw);                                  // barrier B1
    if (tid == e % T) c[e] = ce_new;
    if (tid == 0) {
      b[l] = bl;
      *vp = addmul(*vp, bl, pc);                                                    // :171
      const int32_t pe = perm[e];                                                   // exchangeIndexes :311-320
      perm[e] = perm[n + l];
      perm[n + l] = pe;
    }
    for (int i = tid; i < m; i += T) {
      if (i == l) continue;
      const double ce = col[i];
      A[i * ld + e] = -__ddiv_rn(ce, piv);                                          // :157
      b[i] = submul(b[i], ce, bl);                                                  // :164
    }
    for (int u = wave; u < nq * groups; u += nw) {
      const int j = ((u % nq) << 6) + lane;
      if (j >= n || j == e) continue;
      const double pr = prow[j];
      double* const Aj = A + j;
      const int g = groups;
      int i = u / nq;
      for (; i + 3 * g < m; i += 4 * g) {                                           // :162, four rows in flight
        const int i0 = i, i1 = i + g, i2 = i + 2 * g, i3 = i + 3 * g;
        const double c0 = col[i0], c1 = col[i1], c2 = col[i2], c3 = col[i3];
        const double x0 = submul(Aj[i0 * ld], c0, pr), x1 = submul(Aj[i1 * ld], c1, pr);
        const double x2 = submul(Aj[i2 * ld], c2, pr), x3 = submul(Aj[i3 * ld], c3, pr);
        if (i0 != l) Aj[i0 * ld] = x0;
        if (i1 != l) Aj[i1 * ld] = x1;
        if (i2 != l) Aj[i2 * ld] = x2;
        if (i3 != l) Aj[i3 * ld] = x3;
      }
      for (; i < m; i += g)
        if (i != l) Aj[i * ld] = submul(Aj[i * ld], col[i], pr);
    }
    pivots++;
    __syncthreads();                                                                // barrier B2
  }
  __syncthreads();
  for (int q = tid; q < nvec; q += T) ((d2*)image)[q] = ((const d2*)batch_lds)[q];
  if (tid == 0) {
    a.status[k] = status;
    a.pivots[k] = pivots;
    a.track[k] = track;
  }
}

template <int kThreads>
static hipError_t batch_launch_t(const BatchArgs& a, hipStream_t s) {
  // more than 64 KiB of dynamic LDS has to be asked for per kernel; the launch itself reports what the runtime refuses
  (void)hipFuncSetAttribute((const void*)k_batch_simplex<kThreads>, hipFuncAttributeMaxDynamicSharedMemorySize, a.lds_bytes);
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_batch_simplex<kThreads>, dim3(a.count), dim3(a.threads), (size_t)a.lds_bytes, s, a);
  return hipGetLastError();
}

hipError_t launch_batch_simplex(const BatchArgs& a, hipStream_t s) {
  if (a.count <= 0) return hipSuccess;
  if (a.threads <= 64) return batch_launch_t<64>(a, s);
  if (a.threads <= 256) return batch_launch_t<256>(a, s);
  return batch_launch_t<1024>(a, s);
}

int batch_blocks_per_cu(int threads, int lds_bytes) {
  int nb = 0;
  hipError_t e;
  if (threads <= 64) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_batch_simplex<64>, threads, (size_t)lds_bytes);
  else if (threads <= 256) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_batch_simplex<256>, threads, (size_t)lds_bytes);
  else e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_batch_simplex<1024>, threads, (size_t)lds_bytes);
  if (e != hipSuccess) { (void)hipGetLastError(); return 0; }
  return nb;
}
