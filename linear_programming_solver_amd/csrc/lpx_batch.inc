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

// One LP in LDS as the loop and the pivot see it: pointers into the workgroup's LDS, the row pitch, the CURRENT number of
// columns (k_batch_solve changes it between the phases) and the thread's place in the workgroup.
struct BatchLp {
  double *A, *b, *c, *vp, *col;
  int32_t* perm;
  RatioRow *sh_e, *sh_l;   // 16 entries each: the per-wave partials of the entering and of the leaving reduction
  int ld, m, n;
  int tid, T, lane, wave, nw;
  int dantzig;
};

// the LP of layout L (m rows, n_cur columns now) in the workgroup's LDS, as thread tid of T sees it
__device__ __forceinline__ BatchLp batch_lp(double* lds, const BatchLayout& L, int m, int n_cur, int tid, int T, int dantzig) {
  BatchLp S;
  S.A = lds;
  S.b = lds + L.b;
  S.c = lds + L.c;
  S.vp = lds + L.v;
  S.perm = (int32_t*)(lds + L.perm);
  S.col = lds + L.col;
  S.sh_e = (RatioRow*)(S.col + ((m + 1) & ~1));
  S.sh_l = S.sh_e + 16;
  S.ld = (int)L.ld; S.m = m; S.n = n_cur;
  S.tid = tid; S.T = T; S.lane = tid & 63; S.wave = tid >> 6; S.nw = T >> 6;
  S.dantzig = dantzig;
  return S;
}

// getEntering() over the whole of c (LPState.java:274-285): one barrier
__device__ __forceinline__ RatioRow batch_entering(const BatchLp& S) {
  RatioRow ent = rr_none();
  for (int j = S.tid; j < S.n; j += S.T) batch_consider(ent, S.c[j], j, S.dantzig);
  return batch_reduce(ent, S.sh_e, S.lane, S.wave, S.nw);
}

// col[i] = A[i][e] for a pivot that no ratio test precedes (the forced and the degenerate pivot of phase 1): one barrier
__device__ __forceinline__ void batch_save_column(const BatchLp& S, int e) {
  for (int i = S.tid; i < S.m; i += S.T) S.col[i] = S.A[i * S.ld + e];
  __syncthreads();
}

// pivot(e, l), LPState.java:133-181, on an LP whose column e stands in col[] (visible to every thread).  Returns the
// entering choice of the NEXT iteration, folded from the new c on the way; ends behind barrier B2.
__device__ __forceinline__ RatioRow batch_pivot(const BatchLp& S, int e, int l) {
  double* const A = S.A;
  double* const b = S.b;
  double* const c = S.c;
  const double* const col = S.col;
  const int ld = S.ld, m = S.m, n = S.n, tid = S.tid, T = S.T, lane = S.lane, wave = S.wave, nw = S.nw;
  const int dantzig = S.dantzig;
  const int nq = (n + 63) >> 6;
  const int groups = nq > 0 && nw > nq ? nw / nq : 1;
  // piv, pc and b[l] are read here by every thread; their new values are stored behind barrier B1 only
  const double piv = col[l], pc = c[e];
  const double bl = __ddiv_rn(b[l], piv);                                           // :146
  double* const prow = A + l * ld;
  double ce_new = 0.0;
  RatioRow ent = rr_none();
  for (int j = tid; j < n; j += T) {
    if (j == e) {
      prow[j] = __ddiv_rn(1.0, piv);                                                // :139
      ce_new = -__ddiv_rn(pc, piv);                                                 // :172
      batch_consider(ent, ce_new, j, dantzig);
    } else {
      const double pr = __ddiv_rn(prow[j], piv);                                    // :144
      const double cn = submul(c[j], pc, pr);                                       // :177
      prow[j] = pr;
      c[j] = cn;
      batch_consider(ent, cn, j, dantzig);
    }
  }
  ent = batch_reduce(ent, S.sh_e, lane, wave, nw);                                  // barrier B1
  if (tid == e % T) c[e] = ce_new;
  if (tid == 0) {
    b[l] = bl;
    *S.vp = addmul(*S.vp, bl, pc);                                                  // :171
    const int32_t pe = S.perm[e];                                                   // exchangeIndexes :311-320
    S.perm[e] = S.perm[n + l];
    S.perm[n + l] = pe;
  }
  for (int i = tid; i < m; i += T) {
    if (i == l) continue;
    const double ce = col[i];
    A[i * ld + e] = -__ddiv_rn(ce, piv);                                            // :157
    b[i] = submul(b[i], ce, bl);                                                    // :164
  }
  for (int u = wave; u < nq * groups; u += nw) {
    const int j = ((u % nq) << 6) + lane;
    if (j >= n || j == e) continue;
    const double pr = prow[j];
    double* const Aj = A + j;
    const int g = groups;
    int i = u / nq;
    for (; i + 3 * g < m; i += 4 * g) {                                             // :162, four rows in flight
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
  __syncthreads();                                                                  // barrier B2
  return ent;
}

// The loop of LPSolver.simplex (LPSolver.java:101-107; solveAuxLP :142-157 with `track`) from the entering choice `ent`.
// Returns LPX_OPTIMAL, LPX_UNBOUNDED or LPX_PIVOT_LIMIT; `pivots` counts from the caller's value, `track` < 0 follows nothing.
__device__ __forceinline__ int batch_loop(const BatchLp& S, RatioRow ent, int64_t max_pivots, int64_t& pivots, int& track) {
  for (;;) {
    const int e = ent.row == INT_MAX ? -1 : ent.row;                                // :101
    if (e < 0) return 0 /* LPX_OPTIMAL */;
    RatioRow best = rr_none();                                                      // getLeaving, LPState.java:287-305
    for (int i = S.tid; i < S.m; i += S.T) {
      const double aie = S.A[i * S.ld + e];
      S.col[i] = aie;
      const double r = ratio_of(aie, S.b[i]);
      if (r < kInf) best = rr_min(best, RatioRow{r, i, 0});
    }
    best = batch_reduce(best, S.sh_l, S.lane, S.wave, S.nw);                        // barrier L
    if (!(best.ratio < kInf)) return 1 /* LPX_UNBOUNDED */;                         // :103-106
    if (max_pivots >= 0 && pivots >= max_pivots) return 9 /* LPX_PIVOT_LIMIT */;
    const int l = best.row;
    if (track >= 0) {                                                               // LPSolver.java:151-155
      if (e == track) track = l + S.n;
      else if (l + S.n == track) track = e;
    }
    ent = batch_pivot(S, e, l);
    pivots++;
  }
}

template <int kThreads>
__global__ __launch_bounds__(kThreads) void k_batch_simplex(const BatchArgs a) {
  extern __shared__ __attribute__((aligned(16))) double batch_lds[];
  const int k = blockIdx.x;
  if (k >= a.count) return;
  const int m = a.m[k], n = a.n[k];
  const BatchLayout L = batch_layout(m, n);
  const int tid = threadIdx.x, T = blockDim.x;
  if (L.lds_bytes > a.lds_bytes) {  // the host sized the launch from the same formula: never taken, and never out of bounds
    if (tid == 0) { a.status[k] = 7 /* LPX_DEVICE_ERROR */; a.pivots[k] = 0; }
    return;
  }
  double* const image = a.image + a.offset[k];
  const int nvec = (int)(L.image >> 1);
  for (int q = tid; q < nvec; q += T) ((d2*)batch_lds)[q] = ((const d2*)image)[q];

  const BatchLp S = batch_lp(batch_lds, L, m, n, tid, T, a.dantzig);
  __syncthreads();

  int64_t pivots = 0;
  int track = a.track[k];
  const RatioRow ent = batch_entering(S);
  const int status = batch_loop(S, ent, a.max_pivots, pivots, track);
  __syncthreads();
  for (int q = tid; q < nvec; q += T) ((d2*)image)[q] = ((const d2*)batch_lds)[q];
  if (tid == 0) {
    a.status[k] = status;
    a.pivots[k] = pivots;
    a.track[k] = track;
  }
}

// k_batch_solve: the whole of LPSolver.solve (LPSolver.java:78-133) for MANY SMALL standard forms in one launch, one
// workgroup per form.  What it adds around the loop above, all of it on chip and per LP:
//   load       `min` negates c (:86-89, exact); minInB (:375-386) is one workgroup reduction on (b[i], i) from 1e50, so a
//              NaN or a value >= 1e50 is never chosen; no index or a minimum >= 0: the loop alone, as k_batch_simplex
//   aux LP     convertIntoAuxLP (:283-321): A at the pitch of n + 1 columns with column n = -1, c = 0 but c[n] = -1,
//              v = 0, perm = originals | x0 (id n + m) | slacks; c0 stays in LDS for the restore
//   phase 1    the forced pivot (n, minInB) (:138, made whatever the budget), the loop with x0 tracked (:142-157; UNBOUNDED
//              here is LPX_AUX_UNBOUNDED), handleInitialization (:166-180: x0 basic with |b[row]| > 1e-9 is LPX_INFEASIBLE)
//              and the degenerate pivot (:182-198) at the first slot with |A[row][i]| > 1e-9, found by a workgroup minimum
//              on the index; it counts in pivots_phase1 and is not held against the budget (as lpx_solve has it)
//   restore    restoreInitialLP (:200-246) bug for bug, as lpx_restore_initial_lp / k_restore_objective have it: an
//              ordered original variable that is nonbasic at aux slot n is LPX_RESTORE_INDEX_FAULT and leaves the auxiliary
//              state as it is; otherwise x0's column is dropped, thread j accumulates c[j] over the entries in order with
//              the same addmul / __dadd_rn sequence, one thread accumulates v, and perm loses x0's slot
//   phase 2    the loop on the restored m x n LP, budget max(0, max_pivots - pivots_phase1)
// and the final image goes back to HBM: m x n, or the m x (n + 1) auxiliary LP when the solve ended inside phase 1.
// Nothing is shared between workgroups.  The one-off shifts (column drop, perm) are done by single waves on whole rows:
// a wave reads a 64-entry chunk and then writes it one place to the left, chunks in increasing order.

// row[j] = row[j + 1] for from <= j < len - 1, by ONE wave
template <typename V>
__device__ __forceinline__ void batch_wave_shift_left(V* row, int from, int len, int lane) {
  for (int base = from; base < len - 1; base += 64) {
    const int j = base + lane;
    V x = V(0);
    if (j + 1 < len) x = row[j + 1];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // no instruction: the compiler keeps the chunk's reads in
    __builtin_amdgcn_wave_barrier();                         // front of its writes, and a wave runs them in that order
    if (j + 1 < len) row[j] = x;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// The two ends of a solve: where an LP's entries come from and where its result goes.  batch_solve_body below runs
// everything between them and asks its `Ends` for
//   b_at(i), maximize(), host_phase1(), order(), order_len()     what minInB, the guards and the restore read
//   load(S, maximize)                 the slack form (convertIntoSlackForm :248-272) into S, c negated for `min`; ends
//                                     behind a barrier
//   load_aux(S, c0, maximize)         A at the auxiliary pitch with column n = -1, b, and c0 = c negated for `min`
//   store(S) / store_restored(S)      the final m x n state: S in the plain layout / at the auxiliary pitch
//   store_aux(S, L)                   the m x (n + 1) auxiliary LP of a solve that ended inside phase 1
// and writes the seven per-LP scalars through the fields every argument block has under the same names.
//
// BatchImageEnds (k_batch_solve): one HBM image per LP (BatchLayout), read whole and written back whole.
struct BatchImageEnds {
  const BatchSolveArgs& a;
  const int k, m, n;
  double* const image;
  const BatchLayout L0;
  __device__ __forceinline__ BatchImageEnds(const BatchSolveArgs& a_, int k_, int m_, int n_)
      : a(a_), k(k_), m(m_), n(n_), image(a_.image + a_.offset[k_]), L0(batch_layout(m_, n_)) {}
  __device__ __forceinline__ double b_at(int i) const { return image[L0.b + i]; }
  __device__ __forceinline__ bool maximize() const { return a.maximize == nullptr || a.maximize[k] != 0; }
  __device__ __forceinline__ bool host_phase1() const { return a.phase1[k] != 0; }
  __device__ __forceinline__ const int32_t* order() const { return a.order + (int64_t)k * a.order_pitch; }
  __device__ __forceinline__ int order_len() const { return a.order_len[k]; }
  __device__ __forceinline__ void load(const BatchLp& S, bool maximize) const {
    const int nvec = (int)(L0.image >> 1);
    for (int q = S.tid; q < nvec; q += S.T) ((d2*)S.A)[q] = ((const d2*)image)[q];
    __syncthreads();
    if (!maximize)
      for (int j = S.tid; j < n; j += S.T) S.c[j] = -S.c[j];                        // :86-89
    __syncthreads();
  }
  __device__ __forceinline__ void load_aux(const BatchLp& S, double* c0, bool maximize) const {
    const int ld0 = (int)L0.ld, ld = S.ld;
    for (int i = S.wave; i < m; i += S.nw) {
      for (int j = S.lane; j < n; j += 64) S.A[i * ld + j] = image[(int64_t)i * ld0 + j];
      if (S.lane == 0) S.A[i * ld + n] = -1.0;                                      // :293
    }
    for (int i = S.tid; i < m; i += S.T) S.b[i] = image[L0.b + i];
    for (int j = S.tid; j < n; j += S.T) {
      const double cj = image[L0.c + j];
      c0[j] = maximize ? cj : -cj;                                                  // :86-89
    }
  }
  __device__ __forceinline__ void store(const BatchLp& S) const {
    const int nvec = (int)(L0.image >> 1);
    for (int q = S.tid; q < nvec; q += S.T) ((d2*)image)[q] = ((const d2*)S.A)[q];
  }
  // the front of the LDS IS the image of the m x (n + 1) auxiliary LP
  __device__ __forceinline__ void store_aux(const BatchLp& S, const BatchLayout& L) const {
    const int nvec = (int)(L.image >> 1);
    for (int q = S.tid; q < nvec; q += S.T) ((d2*)image)[q] = ((const d2*)S.A)[q];
  }
  // m x n at the auxiliary pitch: entry by entry into batch_layout(m, n)
  __device__ __forceinline__ void store_restored(const BatchLp& S) const {
    const int ld0 = (int)L0.ld, ld = S.ld;
    for (int i = S.wave; i < m; i += S.nw)
      for (int j = S.lane; j < n; j += 64) image[(int64_t)i * ld0 + j] = S.A[i * ld + j];
    for (int i = S.tid; i < m; i += S.T) image[L0.b + i] = S.b[i];
    for (int j = S.tid; j < n; j += S.T) image[L0.c + j] = S.c[j];
    if (S.tid == 0) image[L0.v] = *S.vp;
    int32_t* const g_perm = (int32_t*)(image + L0.perm);
    for (int s = S.tid; s < n + m; s += S.T) g_perm[s] = S.perm[s];
  }
};

// BatchScenarioEnds (k_batch_scenarios): ONE m x n matrix in HBM (row-major at pitch n) for every workgroup, scenario k's
// b at b + k * ldb and c at c + k * ldc (a pitch of 0: one vector for all), bit 0 of flags[k] = maximise, bit 1 = the host's
// minInB verdict; v = 0 and the identity permutation are made on chip.  No image goes back: an m x n final state leaves
// its perm and its solution, straight from LDS -- perm is a permutation, so every original id < n sits in exactly one
// slot and every x[id] is written exactly once (0 from a nonbasic slot, b[row] from a basic row); the auxiliary LP of a
// solve that ended inside phase 1 leaves nothing.
struct BatchScenarioEnds {
  const BatchScenarioArgs& a;
  const int k, m, n;
  const double *const gb, *const gc;
  const int32_t flags;
  __device__ __forceinline__ BatchScenarioEnds(const BatchScenarioArgs& a_, int k_)
      : a(a_), k(k_), m(a_.m), n(a_.n), gb(a_.b + (int64_t)k_ * a_.ldb), gc(a_.c + (int64_t)k_ * a_.ldc), flags(a_.flags[k_]) {}
  __device__ __forceinline__ double b_at(int i) const { return gb[i]; }
  __device__ __forceinline__ bool maximize() const { return (flags & 1) != 0; }
  __device__ __forceinline__ bool host_phase1() const { return (flags & 2) != 0; }
  __device__ __forceinline__ const int32_t* order() const { return a.order; }
  __device__ __forceinline__ int order_len() const { return a.order_len; }
  // one wave per row, 8-byte accesses: the rows of the shared matrix at pitch n into the odd pitch of S
  __device__ __forceinline__ void load_rows(const BatchLp& S) const {
    const int ld = S.ld;
    for (int i = S.wave; i < m; i += S.nw)
      for (int j = S.lane; j < n; j += 64) S.A[i * ld + j] = a.A[(int64_t)i * n + j];
    for (int i = S.tid; i < m; i += S.T) S.b[i] = gb[i];
  }
  __device__ __forceinline__ void load(const BatchLp& S, bool maximize) const {
    load_rows(S);
    for (int j = S.tid; j < n; j += S.T) S.c[j] = maximize ? gc[j] : -gc[j];        // :86-89
    if (S.tid == 0) *S.vp = 0.0;
    for (int s = S.tid; s < n + m; s += S.T) S.perm[s] = s;
    __syncthreads();
  }
  __device__ __forceinline__ void load_aux(const BatchLp& S, double* c0, bool maximize) const {
    load_rows(S);
    for (int i = S.tid; i < m; i += S.T) S.A[i * S.ld + n] = -1.0;                  // :293
    for (int j = S.tid; j < n; j += S.T) c0[j] = maximize ? gc[j] : -gc[j];         // :86-89
  }
  __device__ __forceinline__ void store(const BatchLp& S) const {
    int32_t* const g_perm = a.perm_out ? a.perm_out + (int64_t)k * (n + m) : nullptr;
    double* const g_x = a.x_out ? a.x_out + (int64_t)k * n : nullptr;
    for (int s = S.tid; s < n + m; s += S.T) {
      const int32_t id = S.perm[s];
      if (g_perm) g_perm[s] = id;
      if (g_x && id >= 0 && id < n) g_x[id] = s < n ? 0.0 : S.b[s - n];
    }
  }
  __device__ __forceinline__ void store_aux(const BatchLp&, const BatchLayout&) const {}
  __device__ __forceinline__ void store_restored(const BatchLp& S) const { store(S); }
};

// LPSolver.solve (LPSolver.java:78-133) for the m x n form behind `io`, by the whole workgroup in its LDS
template <typename Ends>
__device__ __forceinline__ void batch_solve_body(double* batch_lds, const Ends& io, const int m, const int n) {
  const auto& a = io.a;
  const int k = io.k, na = n + 1;
  const BatchLayout L0 = batch_layout(m, n);
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = T >> 6;
  const bool maximize = io.maximize();

  // minInB straight from HBM; the front of the LDS (every launch has at least kBatchScratchBytes) is the scratch
  RatioRow mb = rr_none();
  for (int i = tid; i < m; i += T) {
    const double bi = io.b_at(i);
    if (bi < kInf) mb = rr_min(mb, RatioRow{bi, i, 0});
  }
  mb = batch_reduce(mb, (RatioRow*)batch_lds, lane, wave, nw);
  const int mib = mb.row;
  const bool phase1 = mib != INT_MAX && mb.ratio < 0.0;                             // LPSolver.java:119
  const BatchSolveLayout W = batch_solve_layout(m, n);
  const BatchLayout L = phase1 ? W.aux : L0;
  // the host sized the launch and its buffers with the same rule from the same b: never taken, and never out of bounds
  if ((phase1 ? W.lds_bytes : L0.lds_bytes) > a.lds_bytes || phase1 != io.host_phase1()) {
    if (tid == 0) {
      a.status[k] = 7 /* LPX_DEVICE_ERROR */;
      a.phase1_used[k] = 0; a.x0_slot[k] = -1; a.n_final[k] = n; a.pivots1[k] = 0; a.pivots2[k] = 0; a.v[k] = 0.0;
    }
    return;
  }
  __syncthreads();   // the scratch has been read

  BatchLp S = batch_lp(batch_lds, L, m, phase1 ? na : n, tid, T, a.dantzig);

  int status = 0;
  int64_t pivots1 = 0, pivots2 = 0;
  int x0 = -1, n_final = n, none = -1;
  if (!phase1) {
    io.load(S, maximize);                                                           // convertIntoSlackForm (:248-272)
    status = batch_loop(S, batch_entering(S), a.max_pivots, pivots2, none);         // :96-114
    __syncthreads();
    io.store(S);
  } else {
    double* const c0 = batch_lds + W.c0;
    int32_t* const order = (int32_t*)(batch_lds + W.order);
    int32_t* const slot_of = (int32_t*)(batch_lds + W.slot);
    const int n_ord = io.order_len();
    const int32_t* const g_order = io.order();
    const int ld = S.ld;
    // convertIntoAuxLP (:283-321)
    io.load_aux(S, c0, maximize);
    for (int j = tid; j < n; j += T) {
      S.c[j] = 0.0;                                                                 // :299-301
      if (j < n_ord) order[j] = g_order[j];
    }
    if (tid == 0) { S.c[n] = -1.0; *S.vp = 0.0; }
    for (int s = tid; s < na + m; s += T) S.perm[s] = s < n ? s : s == n ? n + m : s - 1;
    __syncthreads();

    // solveAuxLP (:135-164)
    batch_save_column(S, n);
    RatioRow ent = batch_pivot(S, n, mib);                                          // :138
    pivots1 = 1;
    x0 = mib + na;                                                                  // :139
    const int64_t lim1 = a.max_pivots < 0 ? -1 : (a.max_pivots > 1 ? a.max_pivots - 1 : 0);
    int64_t done = 0;
    status = batch_loop(S, ent, lim1, done, x0);
    pivots1 += done;
    if (status == 1) status = 3 /* LPX_AUX_UNBOUNDED */;                            // :147-150
    __syncthreads();
    n_final = na;
    if (status == 0 && x0 >= na) {
      const int row = x0 - na;
      if (fabs(S.b[row]) > kEps) status = 2 /* LPX_INFEASIBLE */;                   // handleInitialization :171-174
      else {
        RatioRow first = rr_none();                                                 // performDegeneratePivot :182-198
        for (int i = tid; i < na; i += T)
          if (fabs(S.A[row * ld + i]) > kEps) first = rr_min(first, RatioRow{0.0, i, 0});
        first = batch_reduce(first, S.sh_l, lane, wave, nw);
        if (first.row == INT_MAX) status = 4 /* LPX_NO_DEGENERATE_PIVOT */;         // :192-194
        else {
          batch_save_column(S, first.row);
          batch_pivot(S, first.row, row);                                           // :195
          pivots1++;
          x0 = first.row;
        }
      }
    }
    if (status == 0) {
      // restoreInitialLP (:200-246).  auxLP.coefficients first: the slot of every original variable
      for (int s = tid; s < na + m; s += T) {
        const int32_t id = S.perm[s];
        if (id >= 0 && id < n) slot_of[id] = s;
      }
      // :231 with cur = n is the reference's ArrayIndexOutOfBoundsException: only the variable in slot n can raise it
      const int32_t at_n = S.perm[n];
      RatioRow fault = rr_none();
      if (at_n >= 0 && at_n < n)
        for (int t = tid; t < n_ord; t += T)
          if (order[t] == at_n) fault = rr_min(fault, RatioRow{0.0, t, 0});
      fault = batch_reduce(fault, S.sh_e, lane, wave, nw);
      if (fault.row != INT_MAX) status = 6 /* LPX_RESTORE_INDEX_FAULT */;
    }
    if (status == 0) {
      for (int i = wave; i < m; i += nw) batch_wave_shift_left(S.A + i * ld, x0, na, lane);          // :208-211
      __syncthreads();
      for (int j = tid; j < n; j += T) {                                            // :213-233, as k_restore_objective
        double acc = 0.0;
        for (int t = 0; t < n_ord; ++t) {
          const int32_t index = order[t];
          const int cur = slot_of[index];                                           // :220
          const double kk = c0[index];                                              // :219
          if (cur >= na) {
            const double coef = -S.A[(cur - na) * ld + j];                          // :226
            acc = addmul(acc, coef, kk);                                            // :227
          } else if (cur == j) {
            acc = __dadd_rn(acc, kk);                                               // :231 (an aux-LP slot as a post-drop index)
          }
        }
        S.c[j] = acc;
      }
      if (tid == T - 1) {
        double v = 0.0;
        for (int t = 0; t < n_ord; ++t) {
          const int32_t index = order[t];
          const int cur = slot_of[index];
          if (cur >= na) v = addmul(v, S.b[cur - na], c0[index]);                   // :223
        }
        *S.vp = v;
      }
      if (wave == 0) batch_wave_shift_left(S.perm, x0, na + m, lane);               // :235-244
      __syncthreads();
      S.n = n;
      n_final = n;
      const int64_t lim2 = a.max_pivots < 0 ? -1 : (a.max_pivots > pivots1 ? a.max_pivots - pivots1 : 0);
      status = batch_loop(S, batch_entering(S), lim2, pivots2, none);               // :96-114
      __syncthreads();
    }
    if (n_final == na) io.store_aux(S, L);   // ended inside phase 1
    else io.store_restored(S);
  }
  if (tid == 0) {
    a.status[k] = status;
    a.phase1_used[k] = phase1 ? 1 : 0;
    a.x0_slot[k] = x0;
    a.n_final[k] = n_final;
    a.pivots1[k] = pivots1;
    a.pivots2[k] = pivots2;
    a.v[k] = *S.vp;
  }
}

template <int kThreads>
__global__ __launch_bounds__(kThreads) void k_batch_solve(const BatchSolveArgs a) {
  extern __shared__ __attribute__((aligned(16))) double batch_lds[];
  const int k = blockIdx.x;
  if (k >= a.count) return;
  const int m = a.m[k], n = a.n[k];
  batch_solve_body(batch_lds, BatchImageEnds(a, k, m, n), m, n);
}

// k_batch_scenarios: k_batch_solve for `count` scenarios of ONE m x n constraint matrix, one workgroup per scenario
// (BatchScenarioEnds above: only b, c and a flag word per scenario come up from HBM, only perm, x and seven scalars go down).
template <int kThreads>
__global__ __launch_bounds__(kThreads) void k_batch_scenarios(const BatchScenarioArgs a) {
  extern __shared__ __attribute__((aligned(16))) double batch_lds[];
  const int k = blockIdx.x;
  if (k >= a.count) return;
  batch_solve_body(batch_lds, BatchScenarioEnds(a, k), a.m, a.n);
}

// ---- re-solve from a shared basis: k_scenarios_crash once per basis, k_batch_resolve per launch of scenarios ------------------
// A scenario sweep is a base case plus perturbations, and the base case's optimal basis is optimal or nearly so for most of
// them.  The crash brings the shared matrix to that basis once and records what its pivots did to b, c and v (the eta file,
// lpx_kernels.h); a scenario replays that in O(m + n) per crash pivot, looks at its b' and c' and takes one of three routes:
//   primal  b' >= 0: the loop above from (A', b', c')
//   dual    some b' < 0 and no c'[j] > 1e-9: batch_dual_loop below until b' >= -1e-9, then the loop above (which normally
//           ends at once).  No auxiliary LP, no restore: phase 1 is never entered
//   cold    neither: the workgroup writes the route and ends; the host solves the scenario from the slack basis
// Every pivot is batch_pivot, so the bits are those of the reference's pivot in either arithmetic mode.

// k_scenarios_crash: ONE workgroup, the matrix in LDS at the odd pitch with b = c = 0, v = 0 and the identity permutation.
// One pass over the slots j = 0..n-1: where perm[j] is wanted, pivot on the largest |A[i][j]| among the rows whose basic
// variable is not wanted (lowest row on ties, a NaN never; none, or a maximum <= 1e-9: the basis is singular at perm[j]).
// One pass is enough: the pivot leaves an unwanted variable in slot j, and a wanted one never leaves the basis.
template <int kThreads>
__global__ __launch_bounds__(kThreads) void k_scenarios_crash(const ScenarioCrashArgs a) {
  extern __shared__ __attribute__((aligned(16))) double batch_lds[];
  const int m = a.m, n = a.n, tid = threadIdx.x, T = blockDim.x;
  const BatchLayout L = batch_layout(m, n);
  if (blockIdx.x != 0) return;
  if (L.lds_bytes > a.lds_bytes) {  // the host sized the launch from the same formula: never taken, and never out of bounds
    if (tid == 0) { a.info[0] = 0; a.info[1] = -2; }
    return;
  }
  const BatchLp S = batch_lp(batch_lds, L, m, n, tid, T, 0);
  const int ld = S.ld;
  for (int i = S.wave; i < m; i += S.nw)
    for (int j = S.lane; j < n; j += 64) S.A[i * ld + j] = a.A[(int64_t)i * n + j];
  for (int i = tid; i < m; i += T) S.b[i] = 0.0;
  for (int j = tid; j < n; j += T) S.c[j] = 0.0;
  if (tid == 0) *S.vp = 0.0;
  for (int s = tid; s < n + m; s += T) S.perm[s] = s;
  __syncthreads();
  const int64_t stride = eta_stride(m, n);
  int t = 0, singular = -1;
  for (int j = 0; j < n; ++j) {
    const int32_t id = S.perm[j];
    if (!a.wanted[id]) continue;
    RatioRow best = rr_none();                          // (-|A[i][j]|, i): the lexicographic minimum is the largest, lowest row
    for (int i = tid; i < m; i += T) {
      const double x = fabs(S.A[i * ld + j]);
      if (x > kEps && !a.wanted[S.perm[n + i]]) best = rr_min(best, RatioRow{-x, i, 0});
    }
    best = batch_reduce(best, S.sh_l, S.lane, S.wave, S.nw);
    if (best.row == INT_MAX) { singular = id; break; }
    const int l = best.row;
    batch_save_column(S, j);
    batch_pivot(S, j, l);
    double* const E = a.eta + t * stride;               // col[] is as saved, row l is the normalised pivot row
    if (tid == 0) { E[0] = (double)j; E[1] = (double)l; E[2] = S.col[l]; E[3] = 0.0; }
    for (int i = tid; i < m; i += T) E[4 + i] = S.col[i];
    for (int q = tid; q < n; q += T) E[4 + m + q] = S.A[l * ld + q];
    ++t;                                                // the next write of col[] stands behind the barrier of batch_reduce
  }
  if (tid == 0) { a.info[0] = t; a.info[1] = singular; }
  if (singular >= 0) return;
  for (int i = S.wave; i < m; i += S.nw)
    for (int j = S.lane; j < n; j += 64) a.A_out[(int64_t)i * n + j] = S.A[i * ld + j];
  for (int s = tid; s < n + m; s += T) a.perm_out[s] = S.perm[s];
}

// What batch_pivot does to b, c and v for every entry of the eta file, in order, on the b and c in LDS; returns v.  One
// barrier per entry: c[e] and b[l] are read by every thread in front of it and written behind it by the threads that own
// them in the strided loops (every thread carries the two new values in registers, should the next entry read them).
// The next entry's header and each thread's first element of its column and row are loaded before the barrier, so their
// latency hides behind the entry at hand.  Ends behind a barrier.
__device__ __forceinline__ double batch_replay(const BatchLp& S, const double* __restrict__ eta, int n_eta) {
  const int m = S.m, n = S.n, tid = S.tid, T = S.T;
  const int64_t stride = eta_stride(m, n);
  const double* E = eta;
  double h0 = 0.0, h1 = 0.0, h2 = 1.0, hc = 0.0, hp = 0.0;
  if (n_eta > 0) {
    h0 = E[0]; h1 = E[1]; h2 = E[2];
    if (tid < m) hc = E[4 + tid];
    if (tid < n) hp = E[4 + m + tid];
  }
  double v = 0.0, ce_new = 0.0, bl_new = 0.0;
  int pe = -1, pl = -1;
  for (int t = 0; t < n_eta; ++t) {
    const int e = (int)h0, l = (int)h1;
    const double piv = h2, col0 = hc, prow0 = hp;
    const double* const col = E + 4;
    const double* const prow = col + m;
    E += stride;
    if (t + 1 < n_eta) {
      h0 = E[0]; h1 = E[1]; h2 = E[2];
      if (tid < m) hc = E[4 + tid];
      if (tid < n) hp = E[4 + m + tid];
    }
    const double pc = e == pe ? ce_new : S.c[e];
    const double bl = __ddiv_rn(l == pl ? bl_new : S.b[l], piv);                    // :146
    if (tid < n && tid != e) S.c[tid] = submul(S.c[tid], pc, prow0);                // :177
    for (int j = tid + T; j < n; j += T)
      if (j != e) S.c[j] = submul(S.c[j], pc, prow[j]);
    if (tid < m && tid != l) S.b[tid] = submul(S.b[tid], col0, bl);                 // :164
    for (int i = tid + T; i < m; i += T)
      if (i != l) S.b[i] = submul(S.b[i], col[i], bl);
    v = addmul(v, bl, pc);                                                          // :171
    ce_new = -__ddiv_rn(pc, piv);                                                   // :172
    bl_new = bl;
    pe = e;
    pl = l;
    __syncthreads();
    if (tid == e % T) S.c[e] = ce_new;
    if (tid == l % T) S.b[l] = bl_new;
  }
  __syncthreads();
  return v;
}

// minInB (LPSolver.java:375-386) on the b in LDS: from 1e50, lowest row on ties, a NaN never; one barrier
__device__ __forceinline__ RatioRow batch_min_in_b(const BatchLp& S) {
  RatioRow mb = rr_none();
  for (int i = S.tid; i < S.m; i += S.T) {
    const double bi = S.b[i];
    if (bi < kInf) mb = rr_min(mb, RatioRow{bi, i, 0});
  }
  return batch_reduce(mb, S.sh_l, S.lane, S.wave, S.nw);
}

// The dual simplex loop from a state with no c[j] > 1e-9 and some b[i] < 0.  One iteration: the leaving row l by minInB on
// the current b (not below -1e-9: done, 0); the entering slot e with the smallest c[j] / A[l][j] among A[l][j] < -1e-9, a
// strict < scan from 1e50, lowest slot on ties (none: LPX_INFEASIBLE -- row l says a sum of nonnegative terms is
// negative); the budget, where batch_loop has it (LPX_PIVOT_LIMIT); the pivot.  Row l is contiguous in LDS, so the
// ratio scan is conflict-free.  Five barriers per iteration.
__device__ __forceinline__ int batch_dual_loop(const BatchLp& S, int64_t max_pivots, int64_t& pivots) {
  for (;;) {
    const RatioRow mb = batch_min_in_b(S);
    if (mb.row == INT_MAX || !(mb.ratio < -kEps)) return 0;
    const int l = mb.row;
    const double* const row = S.A + l * S.ld;
    RatioRow best = rr_none();
    for (int j = S.tid; j < S.n; j += S.T) {
      const double alj = row[j];
      if (alj < -kEps) {
        const double r = __ddiv_rn(S.c[j], alj);
        if (r < kInf) best = rr_min(best, RatioRow{r, j, 0});
      }
    }
    best = batch_reduce(best, S.sh_e, S.lane, S.wave, S.nw);
    if (best.row == INT_MAX) return 2 /* LPX_INFEASIBLE */;
    if (max_pivots >= 0 && pivots >= max_pivots) return 9 /* LPX_PIVOT_LIMIT */;
    batch_save_column(S, best.row);
    batch_pivot(S, best.row, l);
    pivots++;
  }
}

// k_batch_resolve: one workgroup per scenario, LDS of batch_layout(m, n) -- no auxiliary layout is ever needed.
template <int kThreads>
__global__ __launch_bounds__(kThreads) void k_batch_resolve(const BatchResolveArgs a) {
  extern __shared__ __attribute__((aligned(16))) double batch_lds[];
  const int k = blockIdx.x;
  if (k >= a.count) return;
  const int m = a.m, n = a.n, tid = threadIdx.x, T = blockDim.x;
  const BatchLayout L = batch_layout(m, n);
  if (L.lds_bytes > a.lds_bytes) {  // the host sized the launch from the same formula: never taken, and never out of bounds
    if (tid == 0) {
      a.route[k] = 1;
      a.status[k] = 7 /* LPX_DEVICE_ERROR */;
      a.phase1_used[k] = 0; a.x0_slot[k] = -1; a.n_final[k] = n; a.pivots1[k] = 0; a.pivots2[k] = 0; a.v[k] = 0.0;
    }
    return;
  }
  const BatchScenarioEnds io(a, k);
  const BatchLp S = batch_lp(batch_lds, L, m, n, tid, T, a.dantzig);
  const bool maximize = io.maximize();
  for (int i = tid; i < m; i += T) S.b[i] = io.gb[i];
  for (int j = tid; j < n; j += T) S.c[j] = maximize ? io.gc[j] : -io.gc[j];       // :86-89
  __syncthreads();
  const double v0 = batch_replay(S, a.eta, a.n_eta);
  const RatioRow mb = batch_min_in_b(S);
  const bool needs_dual = mb.row != INT_MAX && mb.ratio < 0.0;                      // LPSolver.java:119 at the basis
  RatioRow ent = batch_entering(S);
  if (needs_dual && ent.row != INT_MAX) {
    if (tid == 0) a.route[k] = 0 /* LPX_ROUTE_COLD */;
    return;
  }
  const int ld = S.ld;
  for (int i = S.wave; i < m; i += S.nw)
    for (int j = S.lane; j < n; j += 64) S.A[i * ld + j] = a.A[(int64_t)i * n + j];
  for (int s = tid; s < n + m; s += T) S.perm[s] = a.perm0[s];
  if (tid == 0) *S.vp = v0;
  __syncthreads();
  int status = 0, none = -1;
  int64_t pivots1 = 0, pivots2 = 0;
  if (needs_dual) {
    status = batch_dual_loop(S, a.max_pivots, pivots1);
    if (status == 0) ent = batch_entering(S);
  }
  if (status == 0) {
    const int64_t lim2 = a.max_pivots < 0 ? -1 : (a.max_pivots > pivots1 ? a.max_pivots - pivots1 : 0);
    status = batch_loop(S, ent, lim2, pivots2, none);
  }
  __syncthreads();
  io.store(S);
  if (tid == 0) {
    a.route[k] = needs_dual ? 2 /* LPX_ROUTE_DUAL */ : 1 /* LPX_ROUTE_PRIMAL */;
    a.status[k] = status;
    a.phase1_used[k] = 0;
    a.x0_slot[k] = -1;
    a.n_final[k] = n;
    a.pivots1[k] = pivots1;
    a.pivots2[k] = pivots2;
    a.v[k] = *S.vp;
  }
}

// Host side of the kernels.  K names a kernel template and its argument block; the workgroup size picks the
// instantiation (64, 256, 1024) here and nowhere else.
struct BatchSimplexKernel {
  using Args = BatchArgs;
  template <int kThreads> static const void* fn() { return (const void*)k_batch_simplex<kThreads>; }
};
struct BatchSolveKernel {
  using Args = BatchSolveArgs;
  template <int kThreads> static const void* fn() { return (const void*)k_batch_solve<kThreads>; }
};
struct BatchScenarioKernel {
  using Args = BatchScenarioArgs;
  template <int kThreads> static const void* fn() { return (const void*)k_batch_scenarios<kThreads>; }
};

struct ScenarioCrashKernel {
  using Args = ScenarioCrashArgs;
  template <int kThreads> static const void* fn() { return (const void*)k_scenarios_crash<kThreads>; }
};
struct BatchResolveKernel {
  using Args = BatchResolveArgs;
  template <int kThreads> static const void* fn() { return (const void*)k_batch_resolve<kThreads>; }
};

template <typename K>
static const void* batch_kernel(int threads) {
  return threads <= 64 ? K::template fn<64>() : threads <= 256 ? K::template fn<256>() : K::template fn<1024>();
}

template <typename K>
static hipError_t batch_launch(const typename K::Args& a, hipStream_t s) {
  if (a.count <= 0) return hipSuccess;
  const void* const kernel = batch_kernel<K>(a.threads);
  // more than 64 KiB of dynamic LDS has to be asked for per kernel; the launch itself reports what the runtime refuses
  (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, a.lds_bytes);
  (void)hipGetLastError();
  void* params[] = {(void*)&a};
  (void)hipLaunchKernel(kernel, dim3(a.count), dim3(a.threads), params, (size_t)a.lds_bytes, s);
  return hipGetLastError();
}

template <typename K>
static int batch_occupancy(int threads, int lds_bytes) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, batch_kernel<K>(threads), threads, (size_t)lds_bytes) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return nb;
}

hipError_t launch_batch_simplex(const BatchArgs& a, hipStream_t s) { return batch_launch<BatchSimplexKernel>(a, s); }
int batch_blocks_per_cu(int threads, int lds_bytes) { return batch_occupancy<BatchSimplexKernel>(threads, lds_bytes); }
hipError_t launch_batch_solve(const BatchSolveArgs& a, hipStream_t s) { return batch_launch<BatchSolveKernel>(a, s); }
int batch_solve_blocks_per_cu(int threads, int lds_bytes) { return batch_occupancy<BatchSolveKernel>(threads, lds_bytes); }
hipError_t launch_batch_scenarios(const BatchScenarioArgs& a, hipStream_t s) { return batch_launch<BatchScenarioKernel>(a, s); }
int batch_scenarios_blocks_per_cu(int threads, int lds_bytes) { return batch_occupancy<BatchScenarioKernel>(threads, lds_bytes); }
hipError_t launch_scenarios_crash(const ScenarioCrashArgs& a, hipStream_t s) { return batch_launch<ScenarioCrashKernel>(a, s); }
hipError_t launch_batch_resolve(const BatchResolveArgs& a, hipStream_t s) { return batch_launch<BatchResolveKernel>(a, s); }
int batch_resolve_blocks_per_cu(int threads, int lds_bytes) { return batch_occupancy<BatchResolveKernel>(threads, lds_bytes); }
