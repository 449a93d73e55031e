// Part of lpx_kernels.hip (included there, inside lpxk::plain / lpxk::fused; not a translation unit of its own):
// THE SWEEPS of blocked pivoting — every entry run through the block's pending pivots in one pass (k_update_tiles,
// k_update_multi, k_sweep32_pull, k_sweep64_one, k_sweep64_mfma2 and their pack kernels) and the fix-up of the block's
// entering columns and pivot rows (k_block_fixup, k_block_fixup_scatter).  DESIGN.md 3d, 3e.
// The sweep is a pure streaming kernel: x -= col_s[i] * prow_s[j] for the valid pending pivots s, in order, for
// EVERY entry — also at the few positions where a pivot does something else (its own row becomes the normalised
// row, its entering column becomes -(col/p)).  Those positions (K rows and K columns) are recomputed afterwards
// by k_block_fixup from the stale values that k_peek_multi / k_pack_multi saved, with the full case analysis;
// no entry depends on another entry, so the garbage written there in between is never read.
// Workgroup = rows_per_tile (<= 64) rows x 512 columns, thread = one 16-byte double2 per row; the thread's
// slices of the K pivot rows stay in registers (2K doubles), the K x rows multipliers of the tile are staged
// once in LDS (coalesced load, broadcast reads); rows go RB at a time to keep RB loads in flight per thread.
// Cost: two fp64 VALU operations per entry per pivot (the product and the difference must stay two roundings,
// so no FMA): measured ~8 cycles per wave-instruction, which makes the sweep VALU-bound from K ~ 16 on
// (cfg4: 1.36 ms for one pass, 1.55 ms at K = 16, 2.4 ms at K = 32; a one-double-per-thread variant with
// twice the occupancy was not faster).
constexpr int kSweepMaxRows = 128;
#ifndef LPX_SWEEP_NBUF
#define LPX_SWEEP_NBUF 2   // register buffers of the sweep: batches in flight = NBUF - 1 (3: measured 4 % slower, DESIGN 3a)
#endif

// Number of valid leading pending pivots (slots >= kmax were not decided this block): one parallel look at the
// ring by the first wave instead of a chain of dependent loads.  Result valid in every thread.
__device__ __forceinline__ int ring_count(const LpxCtl* __restrict__ ring, int kcap, int kmax, int* sh_np) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const bool ok = lane < kcap && lane < kmax && ring[lane].do_update != 0;
    const unsigned long long mask = __ballot(ok);
    if (lane == 0) *sh_np = (~mask == 0ull) ? 64 : (__ffsll((long long)~mask) - 1);
  }
  __syncthreads();
  return *sh_np;
}
// ... of a ring half of up to 128 slots (blocks of 65..128 pivots): two looks
__device__ __forceinline__ int ring_count128(const LpxCtl* __restrict__ ring, int kmax, int* sh_np) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const unsigned long long m0 = __ballot(lane < kmax && ring[lane].do_update != 0);
    const unsigned long long m1 = __ballot(lane + 64 < kmax && ring[lane + 64].do_update != 0);
    const int n0 = (~m0 == 0ull) ? 64 : (__ffsll((long long)~m0) - 1);
    const int n1 = (~m1 == 0ull) ? 64 : (__ffsll((long long)~m1) - 1);
    if (lane == 0) *sh_np = n0 < 64 ? n0 : 64 + n1;
  }
  __syncthreads();
  return *sh_np;
}

// The K-fold update of one batch of RB rows x one double2 held in registers; the multipliers come from LDS
// (one 16-byte broadcast read = two rows).  PIPE: the steady-state form — straight-line code with the LDS reads of
// step s+D issued before the arithmetic of step s (the compiler, minimising registers, otherwise puts every read
// right in front of its use and the wave eats the full LDS latency 2K times per batch — measured: the fp64 VALU then
// idles half of the time).  In a partly filled block (the tail of a pivot budget, the end of the LP) the steps
// s >= np are skipped by a wave-uniform scalar branch per step; their read-ahead still runs (sh_col is filled for all
// K steps).
enum SweepMode { kSweepSimple = 0, kSweepAll = 1, kSweepGuarded = 2 };
template <int K, int RB, int MODE>
__device__ __forceinline__ void sweep_apply(d2 (&x)[RB], const d2 (&pr)[K], const double (*sh_col)[kSweepMaxRows],
                                            int np, int r0) {
  if constexpr (MODE != kSweepSimple) {
#ifndef LPX_SWEEP_D
#define LPX_SWEEP_D 2
#endif
    constexpr int D = LPX_SWEEP_D;  // read-ahead distance in steps (1, 3 and 4 measured the same or worse)
    d2 cc[D + 1][RB / 2];
#pragma unroll
    for (int s = 0; s < D && s < K; ++s)
#pragma unroll
      for (int r = 0; r < RB; r += 2)
        cc[s][r / 2] = *reinterpret_cast<const d2*>(&sh_col[s][(r0 + r) & (kSweepMaxRows - 1)]);
#pragma unroll
    for (int s = 0; s < K; ++s) {
      if (s + D < K) {
#pragma unroll
        for (int r = 0; r < RB; r += 2)
          cc[(s + D) % (D + 1)][r / 2] =
              *reinterpret_cast<const d2*>(&sh_col[s + D][(r0 + r) & (kSweepMaxRows - 1)]);
      }
      __builtin_amdgcn_sched_barrier(0);
      // kSweepAll (np == K, the steady state): no branch at all — 32 scalar branches per batch cost 17 % (cfg4 alone
      // in place: 1.64 ms vs 1.91 ms); kSweepGuarded: a wave-uniform branch per step for partly filled blocks
      if (MODE == kSweepAll || s < np) {
#pragma unroll
        for (int r = 0; r < RB; r += 2) {
          const d2 c2 = cc[s % (D + 1)][r / 2];
          x[r].x = submul(x[r].x, c2.x, pr[s].x);                      // LPState.java:162
          x[r].y = submul(x[r].y, c2.x, pr[s].y);
          x[r + 1].x = submul(x[r + 1].x, c2.y, pr[s].x);
          x[r + 1].y = submul(x[r + 1].y, c2.y, pr[s].y);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  } else {
#pragma unroll
    for (int s = 0; s < K; ++s) {
      if (s < np) {  // wave-uniform
#pragma unroll
        for (int r = 0; r < RB; r += 2) {
          const d2 c2 = *reinterpret_cast<const d2*>(&sh_col[s][(r0 + r) & (kSweepMaxRows - 1)]);  // LDS broadcast
          x[r].x = submul(x[r].x, c2.x, pr[s].x);
          x[r].y = submul(x[r].y, c2.x, pr[s].y);
          x[r + 1].x = submul(x[r + 1].x, c2.y, pr[s].x);
          x[r + 1].y = submul(x[r + 1].y, c2.y, pr[s].y);
        }
      }
    }
  }
}

// The sweep for K <= 16: one workgroup per tile of rows_per_tile (16) rows x 512 columns.  With at most 16 pivot-row
// slices per thread the kernel keeps three waves per SIMD and is HBM-bound (5.6 TB/s); the long-run form below, built
// for K = 32, measured 14-20 % slower here (cfg4, K = 16, same box: 1.72-1.82 ms vs 1.51 ms) and is not used.
template <int K, bool NT, bool OOP>
__global__ __launch_bounds__(256) void k_update_tiles(double* __restrict__ A, const double* __restrict__ Asrc,
                                                      int64_t ld, int m_local,
                                                      const double* __restrict__ prow_ring,
                                                      const double* __restrict__ col_ring, int64_t mp,
                                                      const LpxCtl* __restrict__ ring, int kmax,
                                                      int rows_per_tile, int nstrips, unsigned* census) {
  __shared__ __attribute__((aligned(16))) double sh_col[K][kSweepMaxRows];
  __shared__ int sh_np;
  // rows per batch (register budget: 2K doubles of pivot rows); K = 32 with 8 rows measured 13 % slower (r02)
  constexpr int RB = (K <= 8) ? 8 : 4;
  const int strip = blockIdx.x % nstrips;
  const int tile = blockIdx.x / nstrips;
  const int cj = strip * 512 + 2 * threadIdx.x;
  const bool act = cj < (int)ld;
  const int r_begin = tile * rows_per_tile;
  const int nrows = min(m_local, r_begin + rows_per_tile) - r_begin;
  // uniform tile base (SGPRs) + 32-bit per-lane byte offset: one VGPR per address
  char* const tile_base = reinterpret_cast<char*>(A + (int64_t)r_begin * ld + strip * 512);
  const char* const src_base =
      OOP ? reinterpret_cast<const char*>(Asrc + (int64_t)r_begin * ld + strip * 512) : tile_base;
  const uint32_t row_bytes = (uint32_t)ld * 8u;  // the launcher checks rows_per_tile * ld * 8 < 2^32
  const uint32_t off0 = threadIdx.x * 16u;

  // Prologue: everything the workgroup needs is requested at once — the ring's flags, the multipliers, the
  // thread's slices of the K pivot rows and the first batch of rows — ONE memory round trip, not four.
  bool ok = false;
  if (threadIdx.x < 64) ok = (int)threadIdx.x < K && (int)threadIdx.x < kmax && ring[threadIdx.x].do_update != 0;
  for (int idx = threadIdx.x; idx < K * kSweepMaxRows; idx += blockDim.x) {
    const int sidx = idx / kSweepMaxRows, r = idx % kSweepMaxRows;
    sh_col[sidx][r] = (r < nrows) ? col_ring[(int64_t)sidx * mp + r_begin + r] : 0.0;  // slots >= np: never used
  }
  d2 pr[K];
#pragma unroll
  for (int s = 0; s < K; ++s)
    pr[s] = act ? *reinterpret_cast<const d2*>(prow_ring + (int64_t)s * ld + cj) : d2{0.0, 0.0};
  // Full strips (all but possibly the last one of a row) with at least one full batch take the fast path below.
  const bool fast_geom = (strip + 1) * 512 <= (int)ld && nrows >= RB;
  // NB register buffers of RB rows each: while one batch is computed, the next NB-1 are in flight (the kernel's time
  // was T_hbm + ~0.55 T_valu with one batch ahead: too few bytes in flight to keep HBM busy during the fp64 work)
  constexpr int NB = (K >= 32) ? LPX_SWEEP_NBUF : 2;  // K = 16: a third buffer would cost the third wave per SIMD
  const int nfull_geom = fast_geom ? nrows / RB : 0;
  d2 xb[NB][RB];
#pragma unroll
  for (int u = 0; u + 1 < NB; ++u) {
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      xb[u][r] = d2{0.0, 0.0};
      if (u < nfull_geom) {  // uniform
        const d2* q = reinterpret_cast<const d2*>(src_base + (off0 + (uint32_t)(u * RB + r) * row_bytes));
        xb[u][r] = NT ? __builtin_nontemporal_load(q) : *q;
      }
    }
  }
  if (threadIdx.x < 64) {
    const unsigned long long mask = __ballot(ok);
    if (threadIdx.x == 0) sh_np = (~mask == 0ull) ? 64 : (__ffsll((long long)~mask) - 1);
  }
  __syncthreads();  // sh_col and sh_np complete
  const int np = sh_np;
  if (np == 0 && !OOP) return;  // out of place: the tableau still has to be carried over

  if (census && blockIdx.x % 509u == 0 && threadIdx.x == 0) atomicOr(census, 1u << xcc_id());  // placement sample

  // Fast path, the steady state: straight-line batches without any per-lane guard, software-pipelined — the next
  // batch's loads are in flight while this one runs its 2 np fp64 operations per entry.
  const int full = np > 0 ? nfull_geom : 0;
  auto stream_batches = [&](auto mode) {
    constexpr int MODE = decltype(mode)::value;
#pragma unroll 1
    for (int bt = 0; bt < full; bt += NB) {
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        if (bt + u < full) {  // uniform
          const int r0 = (bt + u) * RB;
          if (bt + u + NB - 1 < full) {  // request batch bt+u+NB-1 into the buffer that was stored last
#pragma unroll
            for (int r = 0; r < RB; ++r) {
              const d2* q = reinterpret_cast<const d2*>(src_base + (off0 + (uint32_t)(r0 + (NB - 1) * RB + r) * row_bytes));
              xb[(u + NB - 1) % NB][r] = NT ? __builtin_nontemporal_load(q) : *q;
            }
          }
          sweep_apply<K, RB, MODE>(xb[u], pr, sh_col, np, r0);
#pragma unroll
          for (int r = 0; r < RB; ++r) {
            d2* q = reinterpret_cast<d2*>(tile_base + (off0 + (uint32_t)(r0 + r) * row_bytes));
            if (NT) __builtin_nontemporal_store(xb[u][r], q); else *q = xb[u][r];
          }
        }
      }
    }
  };
  if (full > 0) {
    if (np == K) stream_batches(std::integral_constant<int, kSweepAll>{});
    else stream_batches(std::integral_constant<int, kSweepGuarded>{});
  }
  // the rest (partial blocks, rows beyond the last full batch, the partial last strip): guarded
  for (int r0 = full * RB; r0 < nrows; r0 += RB) {
    d2 y[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      y[r] = d2{0.0, 0.0};
      if (r0 + r < nrows && act) {
        const d2* q = reinterpret_cast<const d2*>(src_base + (off0 + (uint32_t)(r0 + r) * row_bytes));
        y[r] = NT ? __builtin_nontemporal_load(q) : *q;
      }
    }
    sweep_apply<K, RB, kSweepSimple>(y, pr, sh_col, np, r0);
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      if (r0 + r < nrows && act) {
        d2* q = reinterpret_cast<d2*>(tile_base + (off0 + (uint32_t)(r0 + r) * row_bytes));
        if (NT) __builtin_nontemporal_store(y[r], q); else *q = y[r];
      }
    }
  }
}

// OOP: read the tableau from Asrc, write the updated one to A (same traffic; lets the NEXT block's decisions read
// the un-updated tableau while this sweep streams — see blocked_loop_overlapped in lpx_engine.cpp).
//
// Work split (round 2): a workgroup owns one 512-column strip and a LONG run of rows (rows_per_wg, several hundred to
// a few thousand) and walks down it in chunks of 64 rows.  Its 2K doubles of pivot-row slices per thread are loaded
// ONCE; per chunk only the K x 64 multipliers (16 KiB at K = 32) are staged — into the other half of the LDS array
// while the current chunk is computed, so a chunk boundary costs one workgroup barrier.  In-kernel timestamps of the
// first version (one workgroup per 64-row tile: profiles/r02_sweep_stamps_before.txt) showed why: inside the batch
// loop a wave spent 0.1 us of 2.2 us per batch waiting for its loads and the SIMD was ~94 % busy with the two waves'
// arithmetic — but a tile's 16 batches took 35 us of the 59 us a workgroup slot was held: the rest was the prologue,
// 128 KiB of pivot-row slices + 16 KiB of multipliers fetched from L2 / Infinity Cache for every 256 KiB of tableau.
constexpr int kSweepChunk = 64;   // rows per chunk; the LDS array holds two chunks' multipliers
#ifndef LPX_SWEEP_LB
#define LPX_SWEEP_LB(K) 2   // waves per SIMD the register allocation is held to (two workgroups per CU)
#endif
static_assert(kSweepMaxRows == 2 * kSweepChunk, "sh_col is double-buffered by chunk");

template <int K, bool NT, bool OOP>
__global__ __launch_bounds__(256, LPX_SWEEP_LB(K)) void k_update_multi(double* __restrict__ A, const double* __restrict__ Asrc,
                                                      int64_t ld, int m_local,
                                                      const double* __restrict__ prow_ring,
                                                      const double* __restrict__ col_ring, int64_t mp,
                                                      const LpxCtl* __restrict__ ring, int kmax,
                                                      int rows_per_wg, int nstrips, unsigned* census, int complement,
                                                      int slot0) {
  // slot0: this pass applies the pending pivots slot0 .. slot0 + K - 1 of the block (a block of more than 32 goes in
  // two passes where the one-pass kernel does not apply); the rings are passed at slot 0, kmax counts from slot 0.
  // complement (0, or 1 + the smallest number of valid pivots at which the steady-state kernel launched in front takes
  // the full strips: 1 for k_sweep32_steady — it takes them always —, 65 for k_sweep64_pipe): only what that kernel
  // leaves is done here.
  __shared__ __attribute__((aligned(16))) double sh_col[K][kSweepMaxRows];
  __shared__ int sh_np;
  constexpr int CH = kSweepChunk;
  if (complement) {
    const int np0 = ring_count(ring, 64, kmax, &sh_np);   // (the kernels in front take blocks of at most 64)
    if (np0 >= complement - 1 && (blockIdx.x % nstrips + 1) * 512 <= (int)ld) return;
    __syncthreads();
  }
  prow_ring += (int64_t)slot0 * ld;
  col_ring += (int64_t)slot0 * mp;
  // rows per batch (register budget: 2K doubles of pivot rows); K = 32 with 8 rows measured 13 % slower (r02)
#ifndef LPX_STRIP_RB
#define LPX_STRIP_RB 4
#endif
#ifndef LPX_STRIP_NB
#define LPX_STRIP_NB 2
#endif
  constexpr int RB = (K <= 8) ? 8 : LPX_STRIP_RB;
  constexpr int NB = LPX_STRIP_NB;                   // register buffers: one batch computed, NB - 1 in flight
  static_assert((CH / RB) % NB == 0, "a chunk holds a whole number of buffer rotations");
  constexpr int PF = (K * CH + 255) / 256;           // multipliers of the next chunk held per thread meanwhile
  const int strip = blockIdx.x % nstrips;
  const int grp = blockIdx.x / nstrips;
  const int cj = strip * 512 + 2 * threadIdx.x;
  const bool act = cj < (int)ld;
  const int r_begin = grp * rows_per_wg;
  const int nrows = min(m_local, r_begin + rows_per_wg) - r_begin;
  if (nrows <= 0) return;
  // uniform run base (SGPRs) + 32-bit per-lane byte offset: one VGPR per address
  char* const tile_base = reinterpret_cast<char*>(A + (int64_t)r_begin * ld + strip * 512);
  const char* const src_base =
      OOP ? reinterpret_cast<const char*>(Asrc + (int64_t)r_begin * ld + strip * 512) : tile_base;
  const uint32_t row_bytes = (uint32_t)ld * 8u;  // the launcher checks rows_per_wg * ld * 8 < 2^32
  const uint32_t off0 = threadIdx.x * 16u;

  // Prologue, once per workgroup: the ring's flags, the first chunk's multipliers, the thread's slices of the K pivot
  // rows and the first batch of rows are requested together — ONE memory round trip, not four.
  bool ok = false, ok_hi = false;   // kmax <= 128 slots: lane u looks at slot u and, in a block of more than 64, at slot 64 + u
  if (threadIdx.x < 64) {
    ok = (int)threadIdx.x < kmax && ring[threadIdx.x].do_update != 0;
    if (kmax > 64) ok_hi = (int)threadIdx.x + 64 < kmax && ring[threadIdx.x + 64].do_update != 0;
  }
  for (int idx = threadIdx.x; idx < K * CH; idx += 256) {
    const int sidx = idx / CH, r = idx % CH;
    sh_col[sidx][r] = (r < nrows) ? col_ring[(int64_t)sidx * mp + r_begin + r] : 0.0;  // slots >= np: never used
  }
  d2 pr[K];
#pragma unroll
  for (int s = 0; s < K; ++s)
    pr[s] = act ? *reinterpret_cast<const d2*>(prow_ring + (int64_t)s * ld + cj) : d2{0.0, 0.0};
  // Full strips (all but possibly the last one of a row) take the pipelined path for their full batches.
  const bool fast_geom = (strip + 1) * 512 <= (int)ld;
  const int nfull_geom = fast_geom ? nrows / RB : 0;   // full batches of the whole run (chunks hold CH / RB each)
  d2 xb[NB][RB];
#pragma unroll
  for (int u = 0; u + 1 < NB; ++u) {
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      xb[u][r] = d2{0.0, 0.0};
      if (u < nfull_geom) {  // uniform
        const d2* q = reinterpret_cast<const d2*>(src_base + (off0 + (uint32_t)(u * RB + r) * row_bytes));
        xb[u][r] = NT ? __builtin_nontemporal_load(q) : *q;
      }
    }
  }
  if (threadIdx.x < 64) {
    const unsigned long long mask = __ballot(ok);
    const unsigned long long mask_hi = kmax > 64 ? __ballot(ok_hi) : 0ull;   // (uniform)
    if (threadIdx.x == 0) {
      int np_block = (~mask == 0ull) ? 64 : (__ffsll((long long)~mask) - 1);   // leading valid slots of the block
      if (np_block == 64) np_block += (~mask_hi == 0ull) ? 64 : (__ffsll((long long)~mask_hi) - 1);
      sh_np = max(0, min(K, np_block - slot0));
    }
  }
  __syncthreads();  // chunk 0's multipliers and sh_np complete
  const int np = sh_np;
  if (np == 0 && !OOP) return;  // out of place: the tableau still has to be carried over

  if (census && blockIdx.x % 61u == 0 && threadIdx.x == 0) atomicOr(census, 1u << xcc_id());  // placement sample
#ifdef LPX_SWEEP_STAMPS   // diagnostic build only: lifetime of sampled workgroups
  long long wg_t0 = wall_clock64();
#endif

  const int full = np > 0 ? nfull_geom : 0;   // batches of the pipelined path, numbered over the whole run
  const int nchunks = (nrows + CH - 1) / CH;
  for (int ch = 0; ch < nchunks; ++ch) {
    const int half = (ch & 1) * CH;                      // this chunk's half of sh_col
    const int c_rows = min(CH, nrows - ch * CH);
    // the next chunk's multipliers: requested now, parked in registers, stored into the other half at the end
    double colpf[PF];
    const bool more = ch + 1 < nchunks;
    if (more) {
      const int n_next = min(CH, nrows - (ch + 1) * CH);
#pragma unroll
      for (int k = 0; k < PF; ++k) {
        const int idx = threadIdx.x + k * 256;
        const int sidx = idx / CH, r = idx % CH;
        colpf[k] = (idx < K * CH && r < n_next) ? col_ring[(int64_t)sidx * mp + r_begin + (ch + 1) * CH + r] : 0.0;
      }
    }
    // pipelined path: straight-line batches without any per-lane guard — the next batch's loads (possibly the next
    // chunk's first rows: the run is contiguous) are in flight while this one runs its 2 np fp64 operations per entry
    const int b_lo = ch * (CH / RB), b_hi = min(full, b_lo + CH / RB);
    auto stream_batches = [&](auto mode) {
      constexpr int MODE = decltype(mode)::value;
#pragma unroll 1
      for (int bt = b_lo; bt < b_hi; bt += NB) {   // b_lo is even: buffer u holds batch bt + u
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          if (bt + u < b_hi) {  // uniform
            const int r0 = (bt + u) * RB;
            if (bt + u + NB - 1 < full) {  // request batch bt+u+NB-1 into the buffer that was stored last
#pragma unroll
              for (int r = 0; r < RB; ++r) {
                const d2* q = reinterpret_cast<const d2*>(src_base + (off0 + (uint32_t)(r0 + (NB - 1) * RB + r) * row_bytes));
                xb[(u + NB - 1) % NB][r] = NT ? __builtin_nontemporal_load(q) : *q;
              }
            }
            sweep_apply<K, RB, MODE>(xb[u], pr, sh_col, np, half + (r0 & (CH - 1)));
#pragma unroll
            for (int r = 0; r < RB; ++r) {
              d2* q = reinterpret_cast<d2*>(tile_base + (off0 + (uint32_t)(r0 + r) * row_bytes));
              if (NT) __builtin_nontemporal_store(xb[u][r], q); else *q = xb[u][r];
            }
          }
        }
      }
    };
    if (b_hi > b_lo) {
      if (np == K) stream_batches(std::integral_constant<int, kSweepAll>{});
      else stream_batches(std::integral_constant<int, kSweepGuarded>{});
    }
    // the rest of the chunk (an empty block carried over out of place, rows beyond the last full batch, the partial
    // last strip): guarded
    const int done_rows = (b_hi > b_lo ? b_hi - b_lo : 0) * RB;
    for (int rr = done_rows; rr < c_rows; rr += RB) {
      const int r0 = ch * CH + rr;
      d2 y[RB];
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        y[r] = d2{0.0, 0.0};
        if (rr + r < c_rows && act) {
          const d2* q = reinterpret_cast<const d2*>(src_base + (off0 + (uint32_t)(r0 + r) * row_bytes));
          y[r] = NT ? __builtin_nontemporal_load(q) : *q;
        }
      }
      sweep_apply<K, RB, kSweepSimple>(y, pr, sh_col, np, half + rr);
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        if (rr + r < c_rows && act) {
          d2* q = reinterpret_cast<d2*>(tile_base + (off0 + (uint32_t)(r0 + r) * row_bytes));
          if (NT) __builtin_nontemporal_store(y[r], q); else *q = y[r];
        }
      }
    }
    if (more) {   // uniform: publish the next chunk's multipliers; everyone is done with the half they go into
#pragma unroll
      for (int k = 0; k < PF; ++k) {
        const int idx = threadIdx.x + k * 256;
        if (idx < K * CH) sh_col[idx / CH][(CH - half) + idx % CH] = colpf[k];
      }
      __syncthreads();
    }
  }
#ifdef LPX_SWEEP_STAMPS
  if (census && blockIdx.x % 16u == 0 && blockIdx.x / 16u < 140 && threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    long long* o = reinterpret_cast<long long*>(census + 8) + (blockIdx.x / 16u) * 2;
    o[0] = wg_t0; o[1] = wall_clock64();
  }
#endif
}

#ifdef LPX_WITH_VARIANTS   // superseded / experiment kernels: csrc/variants/, built by `make variants` only
#define LPX_VARIANT_PART 1
#include "variants/lpx_variants.inc"
#undef LPX_VARIANT_PART
#endif

// ---- the steady state of the sweep with the tableau staged through LDS by LDS-DMA (round 3) -------------------------
// Same work split and arithmetic as k_sweep32_steady; what changes is where a batch waits for the fp64 pipe.  There a
// wave parks its in-flight batches in registers (3 x 16 VGPRs on top of the 128 that hold the pivot-row slices: two
// batches in flight is all the register file allows, and two batches = ~4 us of a SIMD's arithmetic is less than the
// ~5 us the memory system takes under this load).  Here a wave issues global_load_lds_dwordx4 (1 KiB per instruction,
// lane t's 16 bytes land at slot + 16 t) into a ring of NS slots of its OWN in LDS and reads its batch back with one
// ds_read_b128 per row when the batch's turn comes: NS batches in flight per wave, no register parked, and the
// destination of a hand-issued load is LDS, not a VGPR — the compiler has nothing to copy, spill or reuse before the
// data has landed (the hazard class of k_sweep32_steady's register loads, DESIGN.md 3a).  What stays hand-counted is
// vmcnt: the DMA is invisible to the compiler's own bookkeeping, so every read-back sits behind an asm wait with a
// memory clobber.  vmcnt counts this wave's loads, stores and LDS-DMAs in issue order, and "at most N outstanding"
// completes every operation that has at least N younger ones: operations the compiler adds only lengthen a wait; a
// wait is too short only if FEWER operations follow than assumed, which is what the tail counts below are for.
//
// LDS (80 KiB, two workgroups per CU): multipliers [2 chunks][32 pivots][32 rows] = 16 KiB, filled by LDS-DMA too
// (one piece = 4 pivots x 32 rows; each wave brings two pieces of the NEXT chunk right after the chunk barrier), then
// 4 waves x NS slots x 4 KiB.  No slot is shared between waves: the only workgroup barrier is the one per chunk that
// publishes the next chunk's multipliers.
constexpr int kDmaK = 32, kDmaRB = 4, kDmaCH = 32;
#ifndef LPX_DMA_NS
#define LPX_DMA_NS 4
#endif
#ifndef LPX_DMA_DIAG
#define LPX_DMA_DIAG 0   // 1, 2: diagnostic builds of scripts/micro/sweep_dma.hip only (memory pass alone / arithmetic alone)
#endif
constexpr int kDmaNS = LPX_DMA_NS;
constexpr int kDmaMultBytes = 2 * kDmaK * kDmaCH * 8;
constexpr int kDmaSlotBytes = kDmaRB * 64 * 16;
constexpr int kDmaLdsBytes = kDmaMultBytes + 4 * kDmaNS * kDmaSlotBytes;
static_assert(2 * kDmaLdsBytes <= 160 * 1024, "two workgroups per CU");

__device__ __forceinline__ uint32_t lds_addr_of(const void* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)(p);
}
template <int N>
__device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }

// sweep_apply's steady-state form over a linear multiplier image: element (s, row) at mrow[s * STRIDE + row]
template <int K, int RB, int STRIDE>
__device__ __forceinline__ void sweep_apply_lin(d2 (&x)[RB], const d2 (&pr)[K], const double* mrow) {
  constexpr int D = 2;
  d2 cc[D + 1][RB / 2];
#pragma unroll
  for (int s = 0; s < D && s < K; ++s)
#pragma unroll
    for (int r = 0; r < RB; r += 2) cc[s][r / 2] = *reinterpret_cast<const d2*>(mrow + s * STRIDE + r);
#pragma unroll
  for (int s = 0; s < K; ++s) {
    if (s + D < K) {
#pragma unroll
      for (int r = 0; r < RB; r += 2)
        cc[(s + D) % (D + 1)][r / 2] = *reinterpret_cast<const d2*>(mrow + (s + D) * STRIDE + r);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < RB; r += 2) {
      const d2 c2 = cc[s % (D + 1)][r / 2];
      x[r].x = submul(x[r].x, c2.x, pr[s].x);                      // LPState.java:162
      x[r].y = submul(x[r].y, c2.x, pr[s].y);
      x[r + 1].x = submul(x[r + 1].x, c2.y, pr[s].x);
      x[r + 1].y = submul(x[r + 1].y, c2.y, pr[s].y);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

#ifdef LPX_WITH_VARIANTS
#define LPX_VARIANT_PART 2
#include "variants/lpx_variants.inc"
#undef LPX_VARIANT_PART
#endif

// ---- the steady state of the sweep, every wave on its own, batches PULLED in address order (round 3) ----------------
// What bounds k_sweep32_dma is its memory pass: on the same GPU a one-shot copy of the tableau in 4-row x 512-column
// tiles dispatched in address order streams at 6.1 TB/s, the same tiles copied by persistent workgroups that walk
// down their strips at 5.0-5.4 (runs of rows, every G-th tile, any depth of prefetch), and persistent workgroups that
// PULL their next tile from a per-strip counter at 6.0-6.2 (scripts/micro/copy_patterns.hip,
// profiles/r03_copy_patterns.txt): what the hardware dispatcher gives one-shot workgroups for free is that tiles
// are handed out in address order to whoever is free, so the rows in flight chip-wide stay one dense, moving window
// (DRAM pages are used up while they are open); statically assigned rows drift apart.
// So here a WAVE is the worker: it is bound to a 128-column sub-strip (its 32 pivot-row slices stay in registers, as
// before) and takes the next 4-row batch of that sub-strip from the sub-strip's ticket counter.  A batch brings its
// own multipliers (32 pivots x 4 rows = 1 KiB = one LDS-DMA, per-lane source addresses), so nothing is shared between
// the waves of a workgroup: no barrier, no chunk, no run length, no rounds of workgroups, no tail — the grid is
// simply what is resident, and a slow CU pulls fewer tickets.
// Per wave and iteration i (one batch each), everything LDS-DMA / hand-counted as in k_sweep32_dma:
//   wait vmcnt(24)   -> what iteration i-3 issued has landed: the rows and multipliers of batch i, the ticket t(i+3)
//   read batch i from stage slot i % 3 (ds_read_b128 x 4)
//   issue: 4 LDS-DMAs of batch t(i+3) into that slot, 1 LDS-DMA of its multipliers into slot (i+3) % 4, 1 ticket atomic
//   32 steps on batch i, multipliers from slot i % 4;  4 stores
// i.e. 10 operations per iteration, and behind the youngest operation of iteration i-3 that must be complete (its
// atomic) come its 4 stores and 2 x 10: 24.  Whenever one of the last three iterations issued less (start, end of the
// tickets) the wait is vmcnt(0).  The ticket's destination is a VGPR of a hand-issued atomic: it is handed to the
// compiler behind the wait and a scheduling barrier, the same two-statement form as strip_wait4 (DESIGN.md 3a).
constexpr int kPullNS = 3, kPullNM = 4;
constexpr int kPullWaveBytes = kPullNS * kDmaSlotBytes + kPullNM * 1024;   // 16 KiB per wave
static_assert(8 * kPullWaveBytes <= 160 * 1024, "two workgroups per CU");

__device__ __forceinline__ void dma_piece1(const double* p, uint32_t lds) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(p), "s"(lds) : "memory");
}
// one returning atomic add by lane 0; EXEC is saved and restored inside the statement, so the call sites need not run
// with all lanes enabled (they do today: wave-uniform branches only)
__device__ __forceinline__ void ticket_pull(unsigned& tk, unsigned* ctr) {
  const unsigned zero = 0, one = 1;
  unsigned long long keep;
  asm volatile("s_mov_b64 %1, exec\n\ts_mov_b64 exec, 1\n\ts_nop 0\n\tglobal_atomic_add %0, %2, %3, %4 sc0\n\ts_mov_b64 exec, %1"
               : "=v"(tk), "=&s"(keep) : "v"(zero), "v"(one), "s"(ctr) : "memory");
}
__device__ __forceinline__ int ticket_take(unsigned& tk) {   // behind a wait that covers the atomic
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" : "+v"(tk) :: "memory");
  return __builtin_amdgcn_readfirstlane((int)tk);
}

// The multipliers as the pulled batches want them: colT[batch][pivot][row in batch], 1 KiB per batch — ONE contiguous
// LDS-DMA piece, where the ring's [pivot][row] layout makes a batch's multipliers 32 pieces of 32 bytes on 32 different
// lines (measured: the sweep of a block whose multipliers all come from one line ran 9 % faster than a real one).  The
// identity steps of a partly filled block (pivot >= np) get +0 here.  8 MiB at cfg4, a few microseconds in front of the
// sweep on its stream.
// Clock probe (lpx_state_info.sweep_clock_mhz): the FRONT pair of stamps, taken by one workgroup per XCD as the sweep itself
// starts (s_memtime is a per-XCD counter; workgroup i runs on XCD i % 8).  The kernel behind the sweep takes the matching
// pair.  (Until round 5 the pack kernel took it; that kernel now runs on another stream, long before the sweep.)
__device__ __forceinline__ void sweep_front_stamp(long long* __restrict__ clk) {
  if (clk && blockIdx.x < 8 && threadIdx.x == 0) {
    const unsigned x = xcc_id() & 7u;
    clk[x * 4 + 0] = __builtin_amdgcn_s_memtime(); clk[x * 4 + 1] = wall_clock64();
  }
}

template <int KP>
__global__ __launch_bounds__(256) void k_pack_multipliers(const double* __restrict__ col_ring, int64_t mp,
                                                          const LpxCtl* __restrict__ ring, int kmax, int nbt,
                                                          double* __restrict__ colT, unsigned* __restrict__ tickets,
                                                          int nsub, long long* __restrict__ clk) {
  __shared__ int sh_np;
  const int np = ring_count(ring, KP, kmax, &sh_np);
  // clock probe (clk != NULL: the variants library's kernels only — the product's pulled sweeps stamp at their own start,
  // sweep_front_stamp): shader-clock and 100 MHz stamps in front of the sweep; k_block_fixup takes the matching pair behind it
  if (clk && blockIdx.x < 8 && threadIdx.x == 0) {   // (s_memtime is a per-XCD counter: a pair of stamps per XCD, by ONE workgroup of each — workgroup i runs on XCD i % 8)
    const unsigned x = xcc_id() & 7u;
    clk[x * 4 + 0] = __builtin_amdgcn_s_memtime(); clk[x * 4 + 1] = wall_clock64();
  }
  // the sweep's ticket counters start at zero (one per sub-strip, 128 bytes apart): cleared here, in the launch in
  // front of the sweep, instead of by a memset launch of their own
  if (blockIdx.x == 0)
    for (int u = threadIdx.x; u < nsub; u += 256) tickets[u * 32] = 0u;
  const int s = threadIdx.x % KP;
  const int64_t b = (int64_t)blockIdx.x * (256 / KP) + threadIdx.x / KP;
  if (b >= nbt) return;
  d2 lo = d2{0.0, 0.0}, hi = d2{0.0, 0.0};
  if (s < np) {
    const d2* p = reinterpret_cast<const d2*>(col_ring + (int64_t)s * mp + b * 4);   // mp is even: 16-byte aligned
    lo = p[0];
    hi = p[1];
  }
  d2* q = reinterpret_cast<d2*>(colT + b * (KP * 4) + s * 4);
  q[0] = lo;
  q[1] = hi;
}

// one batch: RB = 4 rows (1 KiB each for this wave) and the batch's 1 KiB of packed multipliers
template <bool NT>
__device__ __forceinline__ void dma_batch4m(const char* base, uint32_t o0, uint32_t o1, uint32_t o2, uint32_t o3,
                                            uint32_t lds, const char* mbase, uint32_t lds_m) {
  unsigned keep;
  if (NT)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %6\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %2, %1 nt\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %3, %1 nt\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %4, %1 nt\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %5, %1 nt\n\ts_mov_b32 m0, %8\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %2, %7\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(base), "v"(o0), "v"(o1), "v"(o2), "v"(o3), "s"(lds), "s"(mbase), "s"(lds_m)
                 : "memory", "scc");
  else
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %6\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %2, %1\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %3, %1\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %4, %1\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %5, %1\n\ts_mov_b32 m0, %8\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %2, %7\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(base), "v"(o0), "v"(o1), "v"(o2), "v"(o3), "s"(lds), "s"(mbase), "s"(lds_m)
                 : "memory", "scc");
}

template <bool NT, bool OOP>
__global__ __launch_bounds__(256, 2) void k_sweep32_pull(double* __restrict__ A, const double* __restrict__ Asrc,
                                                         int64_t ld, int m_local,
                                                         const double* __restrict__ prow_ring,
                                                         const double* __restrict__ col_ring, int64_t mp,
                                                         const LpxCtl* __restrict__ ring, int kmax, int nstrips_full,
                                                         const double* __restrict__ col_packed,
                                                         unsigned* __restrict__ tickets, long long* __restrict__ clk) {
  constexpr int K = kDmaK, RB = kDmaRB, NS = kPullNS, NM = kPullNM;
  sweep_front_stamp(clk);
  constexpr int kOps = 2 * RB + 2;                 // per iteration: RB row DMAs, 1 multiplier DMA, 1 atomic, RB stores
  constexpr int kAhead = RB + (NS - 1) * kOps;     // younger than the atomic of iteration i - NS at iteration i's wait
  static_assert(kAhead <= 60, "vmcnt is six bits wide");
  __shared__ __attribute__((aligned(16))) char sm[4 * kPullWaveBytes];
  const int np = ring_count(ring, K, kmax, reinterpret_cast<int*>(sm));
  __syncthreads();   // everyone has read the count before a DMA lands on it
  if (np == 0 && !OOP) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // The grid is G workgroups per strip.  blockIdx % 8 names the XCD's share of the grid; with strip = blockIdx % nstrips
  // an XCD would only see the strips s = x (mod 8), i.e. one eighth of the memory channels (the row pitch is a multiple
  // of the channel interleave).  Shifting each XCD's walk over the strips by x * nstrips / 8 gives every XCD all
  // strips and still every strip G workgroups.
  const int strip = (nstrips_full % 8 == 0)
                        ? (int)(((blockIdx.x >> 3) + (blockIdx.x & 7) * (unsigned)(nstrips_full / 8)) % (unsigned)nstrips_full)
                        : (int)(blockIdx.x % (unsigned)nstrips_full);
  const int sub = strip * 4 + wave;
  const int nbt = m_local / RB;                    // batches of the tableau (m_local % RB == 0: launcher)
  unsigned* const ctr = tickets + sub * 32;        // one counter per sub-strip, 128 bytes apart
  const int64_t row_bytes = ld * 8;
  const int64_t batch_bytes = RB * row_bytes;
  char* const dst_base = reinterpret_cast<char*>(A + sub * 128);
  const char* const src_base = OOP ? reinterpret_cast<const char*>(Asrc + sub * 128) : dst_base;
  const uint32_t off0 = lane * 16u;
  const uint32_t rb32 = (uint32_t)row_bytes;       // 3 rows x ld x 8 < 2^32 (launcher)
  char* const stage = sm + wave * kPullWaveBytes;
  char* const mult = stage + NS * kDmaSlotBytes;
  const uint32_t lds_stage = lds_addr_of(stage), lds_mult = lds_addr_of(mult);
  auto issue = [&](int t, int it) {   // batch t becomes iteration it's: rows -> stage slot it % NS, multipliers -> it % NM
    const char* const base = src_base + (int64_t)t * batch_bytes;                                     // uniform
    const char* const mbase = reinterpret_cast<const char*>(col_packed) + (int64_t)t * 1024;          // uniform
    dma_batch4m<NT>(base, off0, off0 + rb32, off0 + 2 * rb32, off0 + 3 * rb32,
                    (uint32_t)__builtin_amdgcn_readfirstlane((int)(lds_stage + (uint32_t)((it % NS) * kDmaSlotBytes))),
                    mbase, (uint32_t)__builtin_amdgcn_readfirstlane((int)(lds_mult + (uint32_t)((it % NM) * 1024))));
  };

  // prologue: tickets of iterations 0 .. NS-1, their DMAs, the tickets of iterations NS .. 2 NS - 1 (pending), the
  // thread's 32 pivot-row slices; everything is waited for
  unsigned tk[NS];
  int bq[NS + 1];   // bq[k]: the batch of iteration i + k (>= nbt: none)
#pragma unroll
  for (int u = 0; u < NS; ++u) ticket_pull(tk[u], ctr);
  dma_wait<0>();
#pragma unroll
  for (int u = 0; u < NS; ++u) {
    bq[u] = ticket_take(tk[u]);
    if (bq[u] < nbt) issue(bq[u], u);   // uniform
  }
#pragma unroll
  for (int u = 0; u < NS; ++u) ticket_pull(tk[u], ctr);
  d2 pr[K];
#pragma unroll
  for (int s = 0; s < K; ++s) {
    pr[s] = *reinterpret_cast<const d2*>(prow_ring + (int64_t)s * ld + sub * 128 + 2 * lane);
    if (s >= np) pr[s] = d2{0.0, 0.0};   // uniform
  }
  dma_wait<0>();

  int full = 0;   // consecutive most recent iterations that issued all kOps operations
#pragma unroll 1
  for (int i0 = 0;; i0 += NS) {
    if (bq[0] >= nbt) break;   // tickets only grow: nothing is left for this wave (its pending pulls are waited for below)
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const int i = i0 + u;
      const int t = bq[0];
      if (t < nbt) {   // uniform
        // (the first NS iterations need what the prologue issued and waited for)
        if (full >= NS) dma_wait<kAhead>(); else if (i >= NS) dma_wait<0>();
        bq[NS] = ticket_take(tk[u]);   // pulled at iteration i - NS: the batch of iteration i + NS
        const char* const slot = stage + u * kDmaSlotBytes + lane * 16;
        d2 x[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) x[r] = *reinterpret_cast<const d2*>(slot + r * 1024);
        const bool more = bq[NS] < nbt;
        if (more) issue(bq[NS], i + NS);   // refills the slot just read (the statement waits for the reads first)
        else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        ticket_pull(tk[u], ctr);
        full = more ? full + 1 : 0;
#if LPX_DMA_DIAG != 1   // (diagnostic build 1: the memory pass alone)
        sweep_apply_lin<K, RB, RB>(x, pr, reinterpret_cast<const double*>(mult + (i % NM) * 1024));
#endif
        char* const out = dst_base + (int64_t)t * batch_bytes;   // uniform
#pragma unroll
        for (int r = 0; r < RB; ++r) {
          d2* q = reinterpret_cast<d2*>(out + (off0 + (uint32_t)r * rb32));
          if (NT) __builtin_nontemporal_store(x[r], q); else *q = x[r];
        }
      } else {
        bq[NS] = INT_MAX;   // (tickets only grow: what this wave still has pending names nothing either)
      }
#pragma unroll
      for (int k = 0; k < NS; ++k) bq[k] = bq[k + 1];
    }
  }
  dma_wait<0>();   // the pending ticket atomics write registers of this wave: let them land before it ends
}

#ifdef LPX_WITH_VARIANTS   // superseded / experiment kernels: csrc/variants/, built by `make variants` only
#define LPX_VARIANT_PART 3
#include "variants/lpx_variants.inc"
#undef LPX_VARIANT_PART
#endif

// ---- blocks of 33..64 pivots by ONE wave per sub-strip (round 4) -----------------------------------------------------
// k_sweep64_pull needs a PAIR of waves per 128-column sub-strip because 64 pivot-row slices of two doubles do not fit one
// wave.  They do when the sub-strip is 64 columns wide: a lane owns ONE column and keeps its 64 pivot-row values in 128
// VGPRs.  Then the worker is a single wave again and the loop is k_sweep32_pull's, nothing handed over, no second wave
// to wait for: tickets per sub-strip, LDS-DMA staging, hand-counted vmcnt.  What changes with the width:
//   * a batch is 4 rows x 512 bytes; one LDS-DMA instruction (64 lanes x 16 bytes) brings TWO rows — lanes 0..31 the
//     first, lanes 32..63 the second (per-lane offsets) — so a batch is two of them, landing as four contiguous rows;
//   * the batch's multipliers ([pivot][row], 64 x 4 doubles = 2 KiB, the layout k_pack_multipliers<64> writes) are two
//     LDS-DMA instructions; per step the wave reads its four multipliers as two 16-byte broadcasts;
//   * a lane reads and stores 8 bytes per row (ds_read_b64, global_store_dwordx2).
// Per iteration: 2 + 2 LDS-DMAs, 1 ticket atomic, 4 stores = 9 operations; behind the atomic of iteration i - 3 come its
// 4 stores and 2 x 9: vmcnt(22).  With fused arithmetic the 64 steps are 256 v_fma_f64 per batch and wave — the sweep's
// instruction floor at cfg4 is 1.2 ms at 2 GHz against a memory pass of ~1.45 ms for HALF the bytes per pivot of a
// block of 32.  Blocks with fewer than 33 valid pivots, the partial last strip and tableaus whose height is not a
// multiple of 4 are left to the generic kernels, as with k_sweep64_pull.
constexpr int kOneSlotBytes = kDmaRB * 512;                                  // a batch: 4 rows x 64 columns
constexpr int kOneWaveBytes = kPullNS * kOneSlotBytes + kPullNM * 2048;      // 14 KiB per wave
static_assert(8 * kOneWaveBytes <= 160 * 1024, "two workgroups per CU");

// (the instruction offset of an LDS-DMA load moves BOTH addresses: the second KiB of the multipliers needs no M0 step)
template <bool NT>
__device__ __forceinline__ void dma_batch2m2(const char* base, uint32_t o0, uint32_t o1, uint32_t lds, const char* mbase,
                                             uint32_t om, uint32_t lds_m) {
  unsigned keep;
  if (NT)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %2, %1 nt\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %3, %1 nt\n\ts_mov_b32 m0, %7\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %6, %5\n\t"
                 "global_load_lds_dwordx4 %6, %5 offset:1024\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(base), "v"(o0), "v"(o1), "s"(lds), "s"(mbase), "v"(om), "s"(lds_m)
                 : "memory", "scc");
  else
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %2, %1\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %3, %1\n\ts_mov_b32 m0, %7\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %6, %5\n\t"
                 "global_load_lds_dwordx4 %6, %5 offset:1024\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(base), "v"(o0), "v"(o1), "s"(lds), "s"(mbase), "v"(om), "s"(lds_m)
                 : "memory", "scc");
}

// 64 steps on a batch of 4 rows x one column per lane; multipliers [pivot][4 rows] in LDS, read two steps ahead
template <int K>
__device__ __forceinline__ void sweep_apply_one(double (&x)[4], const double (&pr)[K], const double* mrow) {
  constexpr int D = 2;
  d2 cc[D + 1][2];
#pragma unroll
  for (int s = 0; s < D && s < K; ++s) {
    cc[s][0] = *reinterpret_cast<const d2*>(mrow + s * 4);
    cc[s][1] = *reinterpret_cast<const d2*>(mrow + s * 4 + 2);
  }
#pragma unroll
  for (int s = 0; s < K; ++s) {
    if (s + D < K) {
      cc[(s + D) % (D + 1)][0] = *reinterpret_cast<const d2*>(mrow + (s + D) * 4);
      cc[(s + D) % (D + 1)][1] = *reinterpret_cast<const d2*>(mrow + (s + D) * 4 + 2);
    }
    __builtin_amdgcn_sched_barrier(0);
    const d2 c01 = cc[s % (D + 1)][0], c23 = cc[s % (D + 1)][1];
    x[0] = submul(x[0], c01.x, pr[s]);                                             // LPState.java:162
    x[1] = submul(x[1], c01.y, pr[s]);
    x[2] = submul(x[2], c23.x, pr[s]);
    x[3] = submul(x[3], c23.y, pr[s]);
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <bool NT, bool OOP>
__global__ __launch_bounds__(256, 2) void k_sweep64_one(double* __restrict__ A, const double* __restrict__ Asrc,
                                                        int64_t ld, int m_local,
                                                        const double* __restrict__ prow_ring,
                                                        const LpxCtl* __restrict__ ring, int kmax, int nstrips_full,
                                                        const double* __restrict__ col_packed,   // [batch][64][4]
                                                        unsigned* __restrict__ tickets, long long* __restrict__ clk) {
  constexpr int K = 64, RB = kDmaRB, NS = kPullNS, NM = kPullNM;
  sweep_front_stamp(clk);
  constexpr int kOps = 2 + 2 + 1 + RB;             // per iteration: 2 row DMAs, 2 multiplier DMAs, 1 atomic, RB stores
  constexpr int kAhead = RB + (NS - 1) * kOps;     // younger than the atomic of iteration i - NS at iteration i's wait
  static_assert(kAhead <= 60 && RB == 4, "vmcnt is six bits wide; a batch is two two-row DMAs");
  __shared__ __attribute__((aligned(16))) char sm[4 * kOneWaveBytes];
  const int np = ring_count(ring, K, kmax, reinterpret_cast<int*>(sm));
  __syncthreads();   // everyone has read the count before a DMA lands on it
  if (np <= 32) return;   // 0..32 pivots: the generic kernels behind this launch take the block (two passes)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // the grid is G workgroups per group of four sub-strips (256 columns); XCD x walks the groups shifted by
  // x * ngroups / 8 (see k_sweep32_pull)
  const int ngroups = nstrips_full * 2;
  const int grp = (ngroups % 8 == 0)
                      ? (int)(((blockIdx.x >> 3) + (blockIdx.x & 7) * (unsigned)(ngroups / 8)) % (unsigned)ngroups)
                      : (int)(blockIdx.x % (unsigned)ngroups);
  const int sub = grp * 4 + wave;                  // 64-column sub-strip
  const int nbt = m_local / RB;                    // batches of the tableau (m_local % RB == 0: launcher)
  unsigned* const ctr = tickets + sub * 32;        // one counter per sub-strip, 128 bytes apart
  const int64_t row_bytes = ld * 8;
  const int64_t batch_bytes = RB * row_bytes;
  char* const dst_base = reinterpret_cast<char*>(A + sub * 64);
  const char* const src_base = OOP ? reinterpret_cast<const char*>(Asrc + sub * 64) : dst_base;
  const uint32_t rb32 = (uint32_t)row_bytes;       // 3 rows x ld x 8 < 2^32 (launcher)
  const uint32_t off_r = (uint32_t)(lane >> 5) * rb32 + (uint32_t)(lane & 31) * 16u;   // DMA: two rows per instruction
  const uint32_t off_m = (uint32_t)lane * 16u;
  const uint32_t off_x = (uint32_t)lane * 8u;      // the lane's column inside a row of the sub-strip
  char* const stage = sm + wave * kOneWaveBytes;
  char* const mult = stage + NS * kOneSlotBytes;
  const uint32_t lds_stage = lds_addr_of(stage), lds_mult = lds_addr_of(mult);
  auto issue = [&](int t, int it) {   // batch t becomes iteration it's: rows -> stage slot it % NS, multipliers -> it % NM
    const char* const base = src_base + (int64_t)t * batch_bytes;                                     // uniform
    const char* const mbase = reinterpret_cast<const char*>(col_packed) + (int64_t)t * 2048;          // uniform
    dma_batch2m2<NT>(base, off_r, off_r + 2 * rb32,
                     (uint32_t)__builtin_amdgcn_readfirstlane((int)(lds_stage + (uint32_t)((it % NS) * kOneSlotBytes))),
                     mbase, off_m, (uint32_t)__builtin_amdgcn_readfirstlane((int)(lds_mult + (uint32_t)((it % NM) * 2048))));
  };

  // prologue: tickets of iterations 0 .. NS-1, their DMAs, the tickets of iterations NS .. 2 NS - 1 (pending), the
  // lane's 64 pivot-row values; everything is waited for
  unsigned tk[NS];
  int bq[NS + 1];   // bq[k]: the batch of iteration i + k (>= nbt: none)
#pragma unroll
  for (int u = 0; u < NS; ++u) ticket_pull(tk[u], ctr);
  dma_wait<0>();
#pragma unroll
  for (int u = 0; u < NS; ++u) {
    bq[u] = ticket_take(tk[u]);
    if (bq[u] < nbt) issue(bq[u], u);   // uniform
  }
#pragma unroll
  for (int u = 0; u < NS; ++u) ticket_pull(tk[u], ctr);
  double pr[K];
#pragma unroll
  for (int s = 0; s < K; ++s) {
    pr[s] = prow_ring[(int64_t)s * ld + sub * 64 + lane];
    if (s >= np) pr[s] = 0.0;   // uniform: identity steps of a partly filled block (multiplier +0 as well)
  }
  dma_wait<0>();

  int full = 0;   // consecutive most recent iterations that issued all kOps operations
#pragma unroll 1
  for (int i0 = 0;; i0 += NS) {
    if (bq[0] >= nbt) break;   // tickets only grow: nothing is left for this wave (its pending pulls are waited for below)
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const int i = i0 + u;
      const int t = bq[0];
      if (t < nbt) {   // uniform
        // (the first NS iterations need what the prologue issued and waited for)
        if (full >= NS) dma_wait<kAhead>(); else if (i >= NS) dma_wait<0>();
        bq[NS] = ticket_take(tk[u]);   // pulled at iteration i - NS: the batch of iteration i + NS
        const char* const slot = stage + u * kOneSlotBytes + off_x;
        double x[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) x[r] = *reinterpret_cast<const double*>(slot + r * 512);
        const bool more = bq[NS] < nbt;
        if (more) issue(bq[NS], i + NS);   // refills the slot just read (the statement waits for the reads first)
        else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        ticket_pull(tk[u], ctr);
        full = more ? full + 1 : 0;
        sweep_apply_one<K>(x, pr, reinterpret_cast<const double*>(mult + (i % NM) * 2048));
        char* const out = dst_base + (int64_t)t * batch_bytes;   // uniform
#pragma unroll
        for (int r = 0; r < RB; ++r) {
          double* q = reinterpret_cast<double*>(out + (off_x + (uint32_t)r * rb32));
          if (NT) __builtin_nontemporal_store(x[r], q); else *q = x[r];
        }
      } else {
        bq[NS] = INT_MAX;   // (tickets only grow: what this wave still has pending names nothing either)
      }
#pragma unroll
      for (int k = 0; k < NS; ++k) bq[k] = bq[k + 1];
    }
  }
  dma_wait<0>();   // the pending ticket atomics write registers of this wave: let them land before it ends
}

// ---- blocks of 33..64 pivots on the matrix cores (round 4; fused-arithmetic mode only) --------------------------------
// v_mfma_f64_16x16x4_f64 computes D[i][j] = fma(A[i][3], B[3][j], fma(A[i][2], B[2][j], fma(A[i][1], B[1][j],
// fma(A[i][0], B[0][j], C[i][j])))) — a chain of fused multiply-adds in k order, bit for bit (measured: 512 000 random
// entries incl. cancellation cases, 0 mismatches; scripts/micro/mfma_f64_order.hip, profiles/r04_mfma_f64_order.txt).
// That chain IS what the fused mode applies to a tableau entry for four consecutive pending pivots: x <- fma(-col_s[i],
// prow_s[j], x).  So with A = the negated multipliers (16 rows x 4 pivots), B = the pivot rows (4 pivots x 16 columns)
// and C = a 16 x 16 tile of the tableau, sixteen MFMAs in pivot order apply a block of 64 to the tile with the bits of 64
// v_fma_f64 steps.  The rate is the vector unit's (MI355X: fp64 matrix = fp64 vector peak); what the matrix path saves
// is everything AROUND the arithmetic: one A operand per lane feeds 1024 multiply-adds, where the vector kernels read
// two 16-byte LDS broadcasts per four (k_sweep64_one is bound by exactly that: LDS issue).
// A wave is bound to a 64-column sub-strip: its B operands — 16 pivot groups x 4 column tiles, one double per lane —
// stay in 128 VGPRs.  It pulls 16-row tiles of the sub-strip from the sub-strip's ticket counter; a tile is 16 x 64
// entries (8 KiB) in the MFMA's C layout (C[4 r + lane / 16][lane % 16] in register r: one global_load_dwordx2 = four
// 128-byte row segments) plus its 8 KiB of negated multipliers in A layout (k_pack_multipliers_mfma: [tile][group][lane],
// lane = 16 k + i; -0.0 for the identity steps of a partly filled block, whose B values are +0.0: fma(-0, +0, x) = x).
// Three tile buffers rotate (ordinary loads, the compiler counts them): while tile t computes its 64 MFMAs, tiles t + 1
// and t + 2 are in flight.  One wave per SIMD (the register file is the budget), LDS unused.
#if LPX_FUSED
typedef double d4v __attribute__((ext_vector_type(4)));

// A operands of the MFMA sweep: colM[(tile * 16 + g) * 64 + 16 k + i] = -col_ring[4 g + k][16 tile + i]
// (pairs != 0, k_sweep64_mfma2: groups 2 p and 2 p + 1 interleaved per lane, colM[(tile * 8 + p) * 128 + 2 lane + (g & 1)], so that
// one 16-byte load per lane brings the A operands of two groups)
__global__ __launch_bounds__(256) void k_pack_multipliers_mfma(const double* __restrict__ col_ring, int64_t mp,
                                                               const LpxCtl* __restrict__ ring, int kmax, int ntiles,
                                                               double* __restrict__ colM, unsigned* __restrict__ tickets,
                                                               int nsub, long long* __restrict__ clk, int pairs) {
  __shared__ int sh_np;
  const int np = ring_count(ring, 64, kmax, &sh_np);
  if (clk && blockIdx.x < 8 && threadIdx.x == 0) {   // (s_memtime is a per-XCD counter: a pair of stamps per XCD, by ONE workgroup of each — workgroup i runs on XCD i % 8)
    const unsigned x = xcc_id() & 7u;
    clk[x * 4 + 0] = __builtin_amdgcn_s_memtime(); clk[x * 4 + 1] = wall_clock64();
  }
  if (blockIdx.x == 0)
    for (int u = threadIdx.x; u < nsub; u += 256) tickets[u * 32] = 0u;
  // one workgroup per tile: thread = (pivot group pair, lane); reads along rows (i fastest): 128-byte segments
  const int tile = blockIdx.x;
  if (tile >= ntiles) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int idx = q * 256 + threadIdx.x;          // 0 .. 1023 = 16 groups x 64 lanes
    const int g = idx >> 6, l = idx & 63, k = l >> 4, i = l & 15;
    const int s = 4 * g + k;
    const double c = s < np ? col_ring[(int64_t)s * mp + (int64_t)tile * 16 + i] : 0.0;
    colM[(int64_t)tile * 1024 + (pairs ? (g >> 1) * 128 + 2 * l + (g & 1) : idx)] = -c;
  }
}

#ifdef LPX_WITH_VARIANTS
#define LPX_VARIANT_PART 4
#include "variants/lpx_variants.inc"
#undef LPX_VARIANT_PART
#endif


// Second form: TWO waves per SIMD.  k_sweep64_mfma keeps the B operands in 128 VGPRs and therefore runs one wave per
// SIMD: while that wave issues a tile's 48 loads and 16 stores and waits for the last MFMAs of a tile, the matrix pipe
// idles (measured: 2.3 ms per 64 pivots at cfg4 against 1.45 ms of arithmetic).  Here a workgroup is bound to a
// 128-column group, its four waves to the two 64-column sub-strips in pairs, and the B operands of both sub-strips live
// in LDS (2 x 32 KiB, [sub-strip][group][column tile][lane]: every MFMA's B is one conflict-free ds_read_b64 with an
// immediate offset); the registers hold three tiles of C and A.  Two workgroups per CU.
// Memory side (second version; the first one lost a third of its time here, profiles/r04_sweep64_mfma2_what_bounds.txt):
//  * buffer addressing — the tile's base in the resource descriptor (SALU), the row group 4 r in the scalar offset, the
//    lane part in ONE 32-bit VGPR, the column tile in the immediate: no per-load 64-bit VALU address, 30 fewer VGPRs;
//  * the ticket is a hand-issued atomic (ticket_pull) taken behind `s_waitcnt vmcnt(48)` = the 32 loads and 16 stores
//    issued after it.  (`if (lane == 0) atomicAdd` compiled to an aggregated atomic followed by `s_waitcnt vmcnt(0)`:
//    every tile drained the wave's whole queue, stores included.)  The compiler does not know of the atomic, so its own
//    counts are one too strict, never too lax;
//  * the loop body is straight-line: the tile of a ticket past the end is CLAMPED to the last tile for its loads (a
//    re-read, two per wave) and the loop is left before its arithmetic, so no conditional load makes the compiler's
//    vmcnt bookkeeping fall back to draining counts.
constexpr int kMfma2LdsBytes = 2 * 16 * 4 * 64 * 8;
static_assert(2 * kMfma2LdsBytes <= 160 * 1024, "two workgroups per CU");
typedef unsigned v2u __attribute__((ext_vector_type(2)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
template <bool NT, bool OOP>
__global__ __launch_bounds__(256, 2) void k_sweep64_mfma2(double* A, const double* Asrc,   // (no __restrict__: see below)
                                                          int64_t ld, int m_local,
                                                          const double* __restrict__ prow_ring,
                                                          const LpxCtl* __restrict__ ring, int kmax, int nstrips_full,
                                                          const double* colM,   // [tile][group][lane]
                                                          unsigned* tickets, int kmin, long long* clk) {
  constexpr int NG = 16, CT = 4;
  constexpr int kRsrcWord3 = 0x00020000;           // raw buffer, 32-bit data format (gfx9 family)
  constexpr int kAuxNt = NT ? 2 : 0;               // cache policy bit 1 = nt
  __shared__ __attribute__((aligned(16))) double sh_b[2 * NG * CT * 64];
  __shared__ int sh_np;
  sweep_front_stamp(clk);
  const int np = ring_count(ring, 64, kmax, &sh_np);
  // kmin = 33: a block of at most 32 valid pivots (it ended early) is left to the generic kernels launched behind; kmin = 1
  // (whole strips only, no such launches): taken here too — the identity steps of a partly filled block are exact
  // (multiplier -0.0 against a pivot-row value of +0.0), whatever their number
  if (np < kmin) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int ngroups = nstrips_full * 4;            // groups of 128 columns
  const int grp = (ngroups % 8 == 0)
                      ? (int)(((blockIdx.x >> 3) + (blockIdx.x & 7) * (unsigned)(ngroups / 8)) % (unsigned)ngroups)
                      : (int)(blockIdx.x % (unsigned)ngroups);
  // ONE ticket counter per 128-column group: ticket T = (16-row block T / 2, 64-column half T % 2), so the two halves of
  // a row's 1 KiB (one DRAM page) are pulled back to back by two waves (second version; with a counter per half the
  // halves of a page were fetched at unrelated times: 5.3 TB/s alone where k_sweep32_pull's 1 KiB segments stream at 6)
  const int ntiles = 2 * (m_local / 16);
  unsigned* const ctr = tickets + grp * 32;
  const int64_t row_bytes = ld * 8;
  char* const dst_base = reinterpret_cast<char*>(A + grp * 128);
  const char* const src_base = OOP ? reinterpret_cast<const char*>(Asrc + grp * 128) : dst_base;
  const uint32_t rb32 = (uint32_t)row_bytes;       // 16 rows x ld x 8 < 2^32 (launcher)
  const uint32_t off_c = (uint32_t)(lane >> 4) * rb32 + (uint32_t)(lane & 15) * 8u;   // row lane / 16, column lane % 16
  const uint32_t off_a = (uint32_t)lane * 8u;
  // the B operands of the group's two halves into LDS: the four waves share the 128 (half, group, column tile) images
  for (int q = wave; q < 2 * NG * CT; q += 4) {
    const int h = q / (NG * CT), g = (q / CT) % NG, ct = q % CT;
    const int s = 4 * g + (lane >> 4);
    sh_b[q * 64 + lane] = s < np ? prow_ring[(int64_t)s * ld + grp * 128 + h * 64 + ct * 16 + (lane & 15)] : 0.0;
  }
  __syncthreads();
  auto load_tile = [&](int t, d4v (&c)[CT], double (&a)[NG]) {
    const int tt = max(0, min(t, ntiles - 1));                          // uniform; past the end: the last tile again
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(src_base) + (int64_t)(tt >> 1) * 16 * row_bytes + (tt & 1) * 512, 0, -1, kRsrcWord3);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        c[ct][r] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rc, off_c + (uint32_t)ct * 128u,
                                                                                    (int)((uint32_t)(4 * r) * rb32), kAuxNt));
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<double*>(colM) + (int64_t)(tt >> 1) * 1024, 0, -1, kRsrcWord3);
#pragma unroll
    for (int p = 0; p < NG / 2; ++p) {   // (k_pack_multipliers_mfma, pairs: the A operands of groups 2 p and 2 p + 1 side by side)
      const v4u x = __builtin_amdgcn_raw_buffer_load_b128(ra, 2u * off_a + (uint32_t)(p & 3) * 1024u, (p >> 2) * 4096, 0);
      a[2 * p] = __builtin_bit_cast(double, v2u{x[0], x[1]});
      a[2 * p + 1] = __builtin_bit_cast(double, v2u{x[2], x[3]});
    }
  };
// scheduling barrier between a tile's loads and the previous tile's arithmetic (without it the compiler sinks the loads
// behind the MFMA chain: three times slower, profiles/r04_sweep64_mfma2_no_sched_barriers.txt)
#define LPX_MFMA_FENCE __builtin_amdgcn_sched_barrier(0)
  auto work_tile = [&](int t, d4v (&c)[CT], const double (&a)[NG]) {
    const double* const bl = sh_b + (max(0, min(t, ntiles - 1)) & 1) * (NG * CT * 64) + lane;
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        c[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[g], bl[(g * CT + ct) * 64], c[ct], 0, 0, 0);
      }
    // the B operands of group g + 1 (two ds_read2st64_b64) are asked for in front of group g's four MFMAs
    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (g + 1 < NG) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    }
    // a ticket past the end: the arithmetic runs on the re-read last tile and the stores are DROPPED by the buffer's range
    // check (num_records 0), so the loop body has no exit but its back edge
    const int tt = max(0, min(t, ntiles - 1));
    char* const out = dst_base + (int64_t)(tt >> 1) * 16 * row_bytes + (tt & 1) * 512;
    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(out, 0, __builtin_amdgcn_readfirstlane((unsigned)t < (unsigned)ntiles ? -1 : 0), kRsrcWord3);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, (double)c[ct][r]), rd, off_c + (uint32_t)ct * 128u,
                                              (int)((uint32_t)(4 * r) * rb32), kAuxNt);
  };
  // A ticket is pulled a whole step before it is taken: pulled in front of step i - 1's loads, taken in front of step i's.
  // vmcnt counts in order, so the wait in front of the take covers exactly what is OLDER than step i - 1's loads, stores and
  // step i's pull (41 operations) — operations that have had a step's arithmetic to complete and that step i's MFMAs need
  // anyway.  (Taken behind the same step's stores, first version, every step ended by waiting for the loads and stores it
  // had just issued.)
  constexpr int kStepOps = 16 + 8 + 16;   // a step's tile loads, A-operand loads and stores
  static_assert(kStepOps + 1 <= 63, "vmcnt is six bits wide");
  auto take = [&](unsigned& tk) -> int {
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(kStepOps + 1) : "memory");
    return ticket_take(tk);
  };
  d4v c0[CT], c1[CT], c2[CT];
  double a0[NG], a1[NG], a2[NG];
  int t0, t1;
  unsigned k0, k1, k2;                  // three ticket registers, rotating with the tile buffers
  {
    ticket_pull(k0, ctr); ticket_pull(k1, ctr);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    t0 = ticket_take(k0); t1 = ticket_take(k1);
  }
  if (t0 >= ntiles) return;
  load_tile(t0, c0, a0);
  load_tile(t1, c1, a1);
  ticket_pull(k2, ctr);                 // the ticket of the tile the loop's first step loads (covered by the wait below)
  // The loop is entered with nothing in flight (once per wave): the compiler's vmcnt bookkeeping at the loop head is
  // then the loop-carried state alone — merged with the prologue's tiles in flight it waited in the first step of EVERY
  // round for loads the previous step had just issued.  (A real s_waitcnt, which the compiler's pass reads.)
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0), expcnt and lgkmcnt untouched
  // Straight-line body, ONE exit at the back edge.  (With `break`s between the steps the compiler folds the exits into
  // one latch block, and its vmcnt bookkeeping then sees paths that skip a step: it waited for the loads the previous
  // step had just issued.)  Tickets only grow, t0 < t1 < ...: once t0 is past the end everything later is.
#pragma unroll 1
  do {
    ticket_pull(k0, ctr);
    const int t2 = take(k2);
    load_tile(t2, c2, a2);
    LPX_MFMA_FENCE;
    work_tile(t0, c0, a0);
    LPX_MFMA_FENCE;
    ticket_pull(k1, ctr);
    const int t3 = take(k0);
    load_tile(t3, c0, a0);
    LPX_MFMA_FENCE;
    work_tile(t1, c1, a1);
    LPX_MFMA_FENCE;
    ticket_pull(k2, ctr);
    const int t4 = take(k1);
    load_tile(t4, c1, a1);
    LPX_MFMA_FENCE;
    work_tile(t2, c2, a2);
    LPX_MFMA_FENCE;
    t0 = t3; t1 = t4;
  } while (t0 < ntiles);
}

#undef LPX_MFMA_FENCE
// ---- k_sweep128_mfma: a block of up to 128 pivots per pass (EXPERIMENTS 000.55; scripts/micro/sweep_mfma128.hip
// compares it bit for bit with two passes of k_sweep64_mfma2).
// Twice the arithmetic per memory pass puts the kernel at the matrix pipe's floor (the projection: 2.63 ms per 128 pivots on 192
// CUs).  What changes against k_sweep64_mfma2:
//  * the B operands of 128 pivots take 64 KiB for ONE 64-column sub-strip: a workgroup (four waves, two workgroups per CU as
//    before) is bound to a sub-strip, not to a 128-column group;
//  * 256 sub-strips at n = 16384 do not divide 2 x 192 resident workgroups, so the binding is not static: a workgroup pulls
//    CHUNKS (sub-strip, row range) from tickets[0] — chunks of one row range are adjacent sub-strips, so the workgroups running
//    side by side still cover whole rows —, loads the sub-strip's B operands if it changed, and its waves pull the chunk's
//    16-row tiles from the chunk's own counter (tickets[32 * (1 + chunk)]);
//  * two tile buffers instead of three (a tile's A operands are 32 doubles per lane: c 2 x 32 + a 2 x 64 VGPRs): the arithmetic of a
//    tile is twice as long, one tile ahead is as much time as two were;
//  * a ticket is pulled a step before it is taken, as there: the wait in front of the take covers the 32 loads, 16 stores and
//    the next pull issued behind it (vmcnt(49)).
// colM[(tile * 16 + g / 2) * 128 + 2 lane + (g & 1)] = -col_ring[4 g + lane / 16][16 tile + lane % 16], g = 0..31 (16 KiB per tile);
// zeroes the nctr ticket counters (128 bytes apart)
__global__ __launch_bounds__(256) void k_pack_multipliers_mfma128(const double* __restrict__ col_ring, int64_t mp,
                                                                  const LpxCtl* __restrict__ ring, int kmax, int ntiles,
                                                                  double* __restrict__ colM, unsigned* __restrict__ tickets, int nctr,
                                                                  long long* __restrict__ clk) {
  __shared__ int sh_np;
  const int np = ring_count128(ring, kmax, &sh_np);
  if (blockIdx.x == 0)
    for (int u = threadIdx.x; u < nctr; u += 256) tickets[u * 32] = 0u;
  // the clock probe: k_sweep128_mfma takes no stamps, so the words of an earlier pulled sweep are cleared here (in a loop
  // call the blocks of more than 64 come first: no stamped sweep of the same call is in flight beside this launch) and
  // lpx_state_info.sweep_clock_mhz says 0 — without a memset packet between the sweeps
  if (clk && blockIdx.x == 0 && threadIdx.x < 32) clk[threadIdx.x] = 0;
  const int tile = blockIdx.x;
  if (tile >= ntiles) return;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int idx = q * 256 + threadIdx.x;          // 0 .. 2047 = 32 groups x 64 lanes
    const int g = idx >> 6, l = idx & 63, k = l >> 4, i = l & 15;
    const int s = 4 * g + k;
    const double c = s < np ? col_ring[(int64_t)s * mp + (int64_t)tile * 16 + i] : 0.0;
    colM[(int64_t)tile * 2048 + (g >> 1) * 128 + 2 * l + (g & 1)] = -c;
  }
}
#define LPX_MFMA_FENCE __builtin_amdgcn_sched_barrier(0)
template <bool NT, bool OOP>
__global__ __launch_bounds__(256, 2) void k_sweep128_mfma(double* A, const double* Asrc,   // (no __restrict__, as k_sweep64_mfma2)
                                                          int64_t ld, int m_local,
                                                          const double* __restrict__ prow_ring,
                                                          const LpxCtl* __restrict__ ring, int kmax, int nsub,
                                                          const double* colM,   // [tile][pair of groups][lane][2]
                                                          unsigned* tickets, int nranges) {
  constexpr int NG = 32, CT = 4;
  constexpr int kRsrcWord3 = 0x00020000;           // raw buffer, 32-bit data format (gfx9 family)
  constexpr int kAuxNt = NT ? 2 : 0;               // cache policy bit 1 = nt
  __shared__ __attribute__((aligned(16))) double sh_b[NG * CT * 64];   // 64 KiB: [group][column tile][lane]
  __shared__ int sh_np, sh_chunk;
  const int np = ring_count128(ring, kmax, &sh_np);
  // no valid pivot (the block behind the one in which the LP ended): in place nothing to do; out of place the tableau still
  // has to be carried over — every step an identity step (multiplier -0.0 against a pivot-row value of +0.0: exact)
  if (np < 1 && !OOP) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int rowblocks = m_local / 16;
  const int per_range = (rowblocks + nranges - 1) / nranges;
  const int nchunks = nsub * nranges;
  const int64_t row_bytes = ld * 8;
  const uint32_t rb32 = (uint32_t)row_bytes;       // 16 rows x ld x 8 < 2^32 (launcher)
  const uint32_t off_c = (uint32_t)(lane >> 4) * rb32 + (uint32_t)(lane & 15) * 8u;   // row lane / 16, column lane % 16
  const uint32_t off_a = (uint32_t)lane * 8u;
  int sub_loaded = -1;
  for (;;) {
    if (threadIdx.x == 0) sh_chunk = (int)atomicAdd(tickets, 1u);
    __syncthreads();
    const int chunk = __builtin_amdgcn_readfirstlane(sh_chunk);
    if (chunk >= nchunks) return;
    const int sub = chunk % nsub, range = chunk / nsub;
    const int rb0 = range * per_range;
    const int ntiles = min(rowblocks, rb0 + per_range) - rb0;   // 16-row tiles of this chunk
    if (sub != sub_loaded) {   // uniform
      for (int q = wave; q < NG * CT; q += 4) {
        const int g = q / CT, ct = q % CT;
        const int s = 4 * g + (lane >> 4);
        sh_b[q * 64 + lane] = s < np ? prow_ring[(int64_t)s * ld + sub * 64 + ct * 16 + (lane & 15)] : 0.0;
      }
      sub_loaded = sub;
    }
    __syncthreads();
    if (ntiles > 0) {
      unsigned* const ctr = tickets + 32 * (1 + chunk);
      char* const dst_base = reinterpret_cast<char*>(A + sub * 64) + (int64_t)rb0 * 16 * row_bytes;
      const char* const src_base = OOP ? reinterpret_cast<const char*>(Asrc + sub * 64) + (int64_t)rb0 * 16 * row_bytes : dst_base;
      const double* const colM0 = colM + (int64_t)rb0 * 2048;
      auto load_tile = [&](int t, d4v (&c)[CT], double (&a)[NG]) {
        const int tt = max(0, min(t, ntiles - 1));                          // uniform; past the end: the last tile again
        const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char*>(src_base) + (int64_t)tt * 16 * row_bytes, 0, -1, kRsrcWord3);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int ct = 0; ct < CT; ++ct)
            c[ct][r] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rc, off_c + (uint32_t)ct * 128u,
                                                                                         (int)((uint32_t)(4 * r) * rb32), kAuxNt));
        const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<double*>(colM0) + (int64_t)tt * 2048, 0, -1, kRsrcWord3);
#pragma unroll
        for (int p = 0; p < NG / 2; ++p) {   // pairs: the A operands of groups 2 p and 2 p + 1 side by side, 1 KiB per pair
          const v4u x = __builtin_amdgcn_raw_buffer_load_b128(ra, 2u * off_a + (uint32_t)(p & 3) * 1024u, (p >> 2) * 4096, 0);
          a[2 * p] = __builtin_bit_cast(double, v2u{x[0], x[1]});
          a[2 * p + 1] = __builtin_bit_cast(double, v2u{x[2], x[3]});
        }
      };
      auto work_tile = [&](int t, d4v (&c)[CT], const double (&a)[NG]) {
        const double* const bl = sh_b + lane;
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
          for (int ct = 0; ct < CT; ++ct)
            c[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[g], bl[(g * CT + ct) * 64], c[ct], 0, 0, 0);
        // the B operands of group g + 1 (two ds_read2st64_b64) are asked for in front of group g's four MFMAs
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          if (g + 1 < NG) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        }
        // a ticket past the end: the arithmetic runs on the re-read last tile and the stores are DROPPED by the buffer's range check
        const int tt = max(0, min(t, ntiles - 1));
        char* const out = dst_base + (int64_t)tt * 16 * row_bytes;
        const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(out, 0, __builtin_amdgcn_readfirstlane((unsigned)t < (unsigned)ntiles ? -1 : 0), kRsrcWord3);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int ct = 0; ct < CT; ++ct)
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, (double)c[ct][r]), rd, off_c + (uint32_t)ct * 128u,
                                                  (int)((uint32_t)(4 * r) * rb32), kAuxNt);
      };
      constexpr int kStepOps = 16 + 16 + 16;   // a step's C loads, A loads and stores
      auto take = [&](unsigned& tk) -> int {
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(kStepOps + 1) : "memory");
        return ticket_take(tk);
      };
      d4v c0[CT], c1[CT];
      double a0[NG], a1[NG];
      unsigned ka, kb = 0;
      ticket_pull(ka, ctr);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      int t0 = ticket_take(ka);
      if (t0 < ntiles) {   // uniform
        load_tile(t0, c0, a0);
        ticket_pull(ka, ctr);                 // the ticket of the tile the loop's first step loads
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): the loop is entered with nothing in flight (see k_sweep64_mfma2)
#pragma unroll 1
        do {
          ticket_pull(kb, ctr);
          const int t1 = take(ka);
          load_tile(t1, c1, a1);
          LPX_MFMA_FENCE;
          work_tile(t0, c0, a0);
          LPX_MFMA_FENCE;
          ticket_pull(ka, ctr);
          const int t2 = take(kb);
          load_tile(t2, c0, a0);
          LPX_MFMA_FENCE;
          work_tile(t1, c1, a1);
          LPX_MFMA_FENCE;
          t0 = t2;
        } while (t0 < ntiles);
      }
      // the last pull's return (and the re-read tile) must have landed before the registers are used again
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("" : "+v"(ka), "+v"(kb) :: "memory");
    }
    __syncthreads();   // every wave is through with sh_b and sh_chunk
  }
}
#undef LPX_MFMA_FENCE
#ifdef LPX_WITH_VARIANTS
#define LPX_VARIANT_PART 7
#include "variants/lpx_variants.inc"
#undef LPX_VARIANT_PART
#endif
#endif  // LPX_FUSED

#ifdef LPX_WITH_VARIANTS   // superseded / experiment kernels: csrc/variants/, built by `make variants` only
#define LPX_VARIANT_PART 5
#include "variants/lpx_variants.inc"
#undef LPX_VARIANT_PART
#endif

// One pivot applied to one value with the reference's full case analysis (LPState.java:139-164): the value at
// row i, column j before pivot r -> after pivot r.
__device__ __forceinline__ double apply_pivot(double v, int i, int j, int l_r, int e_r, double p_r, double ce,
                                              double pr_j) {
  if (i == l_r) return pr_j;                       // pivot row := normalised row (pr_j = 1/p at j == e_r)
  if (j == e_r) return -__ddiv_rn(ce, p_r);        // :157
  return submul(v, ce, pr_j);        // :162
}

// After the sweep: recompute the entering columns (job 0), the pivot rows (job 1) and b (job 2) of the valid
// pending pivots from the saved stale values.  grid = (ceil(max(m, ld)/256), ceil(K / 8), 3): a thread takes EIGHT
// pending pivots' columns (rows) of its row (column) at once, so that a ring value it loads serves eight chains (one
// pivot per thread re-read the K x m / K x ld ring values K times over: 1.6 GB of L2 traffic per block of 64 at cfg4).
// The case analysis of apply_pivot per (pending pivot r, chain q) made the kernel instruction-bound (~7 700 instructions
// per thread for 512 multiply-adds: 215 us per block of 64 at cfg4, and NOT its scattered 8-byte column writes — written to
// a compact image instead it took 195, EXPERIMENTS.md).  None of its tests depends on the thread:
//   * "chain q's pivot entered at (left through) the same slot (row) as pivot r" is a property of the block: one 8-bit
//     mask per r, computed once per workgroup (sh_eq);
//   * "this thread's row (column) is pivot r's own" can only hold in the one wave whose 64 rows (columns) contain it: one
//     __ballot per wave (lane r asks for pivot r), then a scalar bit test per r.
// A step without either is eight multiply-adds on eight LDS values; with one, the old selects behind a uniform branch.
constexpr int kFixChunk = 8;
// The chains of a job: the LAST pending pivot of every distinct key (entering slot / leaving row), in pivot order.  Called
// by the first wave of a workgroup (all 64 lanes) between two barriers; keys[q] = -1 behind the last pivot.
// (up to kBlockMax = 128 pending pivots: lane q looks after pivots q and 64 + q)
__device__ __forceinline__ void fix_pick_chains(const int* keys, int np, int* sh_pick, int* sh_npick) {
  const int q = threadIdx.x;
  const int key = keys[q], key_hi = keys[64 + q];
  bool keep = q < np, keep_hi = 64 + q < np;
  for (int r = q + 1; r < np; ++r) keep = keep && keys[r] != key;
  for (int r = 64 + q + 1; r < np; ++r) keep_hi = keep_hi && keys[r] != key_hi;
  const unsigned long long mask = __ballot(keep), mask_hi = __ballot(keep_hi);
  const unsigned long long below = (1ull << q) - 1ull;
  if (keep) sh_pick[__popcll(mask & below)] = q;
  if (keep_hi) sh_pick[__popcll(mask) + __popcll(mask_hi & below)] = 64 + q;
  const int npick = __popcll(mask) + __popcll(mask_hi);
  if (q < kFixChunk) sh_pick[npick + q] = 0;   // (padding of the last chunk: reads stay inside the ring)
  if (q == 0) *sh_npick = npick;
}
__global__ __launch_bounds__(256) void k_block_fixup(double* __restrict__ A, int64_t ld, int n, int m_local, int row0,
                                                     double* b, const double* __restrict__ prow_ring,
                                                     const double* __restrict__ col_ring,
                                                     const double* __restrict__ col0_ring,
                                                     const double* __restrict__ row0_ring, int64_t mp,
                                                     const LpxCtl* __restrict__ ring, int kmax,
                                                     const double* b_src, long long* __restrict__ clk,
                                                     double* __restrict__ img_col, double* __restrict__ img_row) {
  // img_col / img_row != NULL (the overlapped loop): the chains are computed BESIDE the block's sweep, from ring values
  // only, into compact images [chain][row] / [chain][column]; k_block_fixup_scatter copies them into the tableau once the
  // sweep is through.  b (job 2) is written in place either way: the sweep does not touch it.
  static_assert(kBlockMax == 128, "two words of hit ballots: lane u asks for pending pivots u and 64 + u");
  if (clk && blockIdx.x < 8 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) {
    const unsigned x = xcc_id() & 7u;
    clk[x * 4 + 2] = __builtin_amdgcn_s_memtime(); clk[x * 4 + 3] = wall_clock64();
  }
  __shared__ double sh_p[kBlockMax], sh_bl[kBlockMax];
  __shared__ __attribute__((aligned(16))) double sh_x[kBlockMax][kFixChunk];   // job 0: prow_r[e_s]; job 1: col_r[l_s]   (r: all pivots, s: this chunk's)
  __shared__ int sh_e[kBlockMax], sh_l[kBlockMax], sh_eq[kBlockMax], sh_pick[kBlockMax + kFixChunk];
  __shared__ int sh_np, sh_npick;
  const int s0 = blockIdx.y * kFixChunk, job = blockIdx.z;
  // (the grid is max(m, ld) wide for all three jobs: a workgroup with nothing to do leaves before the ring is looked at)
  if ((int64_t)blockIdx.x * blockDim.x >= (job == 1 ? ld : (int64_t)m_local) || (job == 2 && s0 != 0)) return;
  const int np = ring_count128(ring, kmax, &sh_np);
  if (job == 2 ? s0 != 0 : s0 >= np) return;  // the b job also runs for an empty block (out of place: it copies b)
  if ((int)threadIdx.x < kBlockMax) {   // (slots behind the last pivot: -1, matches nothing)
    const bool live = (int)threadIdx.x < np;
    const LpxCtl& q = ring[live ? threadIdx.x : 0];
    sh_e[threadIdx.x] = live ? q.e_cur : -1;
    sh_l[threadIdx.x] = live ? q.l - row0 : -1;
    sh_p[threadIdx.x] = live ? q.p : 1.0;
    sh_bl[threadIdx.x] = live ? q.bl : 0.0;
  }
  __syncthreads();
  // Pivots that share their entering slot (their leaving row) end in the SAME column (row): a later pivot at the slot
  // restarts the column whatever it held (:157), a later pivot through the row replaces the row (:139-145).  So only the
  // LAST pivot of every slot (row) is a chain here — under the first-positive rule a block of 64 pivots touches 10-15
  // distinct slots and rows (three decisions of four come back to a slot of the last 48), i.e. a quarter of the chains
  // and of the scattered column writes.
  if (job != 2 && threadIdx.x < 64) fix_pick_chains(job == 1 ? sh_l : sh_e, np, sh_pick, &sh_npick);
  __syncthreads();
  const int npick = job == 2 ? 0 : sh_npick;
  if (job != 2 && s0 >= npick) return;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int ns = min(kFixChunk, npick - s0);   // chains of this chunk (job 0 / 1)
  int pk[kFixChunk];                         // their pivots
#pragma unroll
  for (int q = 0; q < kFixChunk; ++q) pk[q] = sh_pick[(job == 2 ? 0 : s0) + q];
  const int lane = threadIdx.x & 63;
  const int t_wave = t - lane;              // the wave's first row (job 0, 2) / column (job 1)
  if (job == 0) {  // entering columns of pending pivots s0 .. s0 + ns - 1, all local rows
    for (int idx = threadIdx.x; idx < np * kFixChunk; idx += blockDim.x) {
      const int r = idx / kFixChunk, q = idx % kFixChunk;
      sh_x[r][q] = q < ns ? prow_ring[(int64_t)r * ld + sh_e[sh_pick[s0 + q]]] : 0.0;
    }
    if ((int)threadIdx.x < np) {   // which chains of the chunk entered at pivot r's slot (the division of :157)
      int mask = 0;
      for (int q = 0; q < ns; ++q) mask |= (sh_e[sh_pick[s0 + q]] == sh_e[threadIdx.x]) << q;
      sh_eq[threadIdx.x] = mask;
    }
    __syncthreads();
    // pivots whose own row is one of this wave's 64 rows (all lanes active here: lane r asks for pivot r)
    const unsigned long long hit = __ballot((unsigned)(sh_l[lane] - t_wave) < 64u);
    const unsigned long long hit_hi = __ballot((unsigned)(sh_l[64 + lane] - t_wave) < 64u);
    if (t < m_local) {
      double v[kFixChunk];
#pragma unroll
      for (int q = 0; q < kFixChunk; ++q) v[q] = q < ns ? col0_ring[(int64_t)pk[q] * mp + t] : 0.0;
      // the ring values of eight steps are requested together (they do not depend on the running values), one batch
      // ahead of the arithmetic that uses them
      double cv[8], cvn[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) cv[u] = (u < np) ? col_ring[(int64_t)u * mp + t] : 0.0;
      for (int r0 = 0; r0 < np; r0 += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) cvn[u] = (r0 + 8 + u < np) ? col_ring[(int64_t)(r0 + 8 + u) * mp + t] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int r = r0 + u;
          if (r < np) {   // (uniform)
            double x[kFixChunk];
#pragma unroll
            for (int q = 0; q < kFixChunk; ++q) x[q] = sh_x[r][q];
            const int eq = __builtin_amdgcn_readfirstlane(sh_eq[r]);
            if (eq == 0 && !(((r < 64 ? hit >> r : hit_hi >> (r - 64))) & 1)) {   // (uniform, the common case) eight plain steps
#pragma unroll
              for (int q = 0; q < kFixChunk; ++q) v[q] = submul(v[q], cv[u], x[q]);                    // :162
            } else {
              const double pr = sh_p[r];
              const bool own = t == sh_l[r];
#pragma unroll
              for (int q = 0; q < kFixChunk; ++q) {
                double nv;
                if ((eq >> q) & 1) nv = -__ddiv_rn(cv[u], pr);                                          // :157
                else nv = submul(v[q], cv[u], x[q]);                                                   // :162
                v[q] = own ? x[q] : nv;   // pivot row := normalised row
              }
            }
          }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) cv[u] = cvn[u];
      }
#pragma unroll
      for (int q = 0; q < kFixChunk; ++q)
        if (q < ns) {
          if (img_col) img_col[(int64_t)(s0 + q) * mp + t] = v[q];
          else A[(int64_t)t * ld + sh_e[pk[q]]] = v[q];
        }
    }
  } else if (job == 1) {  // pivot rows of pending pivots s0 .. (those that live on this shard), all columns
    for (int idx = threadIdx.x; idx < np * kFixChunk; idx += blockDim.x) {
      const int r = idx / kFixChunk, q = idx % kFixChunk;
      const int i = q < ns ? sh_l[sh_pick[s0 + q]] : -1;
      sh_x[r][q] = (i >= 0 && i < m_local) ? col_ring[(int64_t)r * mp + i] : 0.0;
    }
    if ((int)threadIdx.x < np) {   // which chains of the chunk left through pivot r's row (row := normalised row)
      int mask = 0;
      for (int q = 0; q < ns; ++q) mask |= (sh_l[sh_pick[s0 + q]] == sh_l[threadIdx.x]) << q;
      sh_eq[threadIdx.x] = mask;
    }
    __syncthreads();
    // pivots that entered at one of this wave's 64 slots (the division of :157 sits in THAT column)
    const unsigned long long hit = __ballot((unsigned)(sh_e[lane] - t_wave) < 64u);
    const unsigned long long hit_hi = __ballot((unsigned)(sh_e[64 + lane] - t_wave) < 64u);
    if (t < (int)ld) {
      double v[kFixChunk];
#pragma unroll
      for (int q = 0; q < kFixChunk; ++q) v[q] = (q < ns && t < n) ? row0_ring[(int64_t)pk[q] * ld + t] : 0.0;
      double pv[8], pvn[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) pv[u] = (u < np) ? prow_ring[(int64_t)u * ld + t] : 0.0;
      for (int r0 = 0; r0 < np; r0 += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) pvn[u] = (r0 + 8 + u < np) ? prow_ring[(int64_t)(r0 + 8 + u) * ld + t] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int r = r0 + u;
          if (r < np) {   // (uniform)
            double x[kFixChunk];
#pragma unroll
            for (int q = 0; q < kFixChunk; ++q) x[q] = sh_x[r][q];
            const int eq = __builtin_amdgcn_readfirstlane(sh_eq[r]);
            if (eq == 0 && !(((r < 64 ? hit >> r : hit_hi >> (r - 64))) & 1)) {
#pragma unroll
              for (int q = 0; q < kFixChunk; ++q) v[q] = submul(v[q], x[q], pv[u]);
            } else {
              const double pr = sh_p[r];
              const bool own = t == sh_e[r];   // (one thread of the grid per pivot r)
#pragma unroll
              for (int q = 0; q < kFixChunk; ++q) {
                double nv;
                if (own) nv = -__ddiv_rn(x[q], pr);
                else nv = submul(v[q], x[q], pv[u]);
                v[q] = ((eq >> q) & 1) ? pv[u] : nv;
              }
            }
          }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) pv[u] = pvn[u];
      }
#pragma unroll
      for (int q = 0; q < kFixChunk; ++q) {
        const int i = q < ns ? sh_l[pk[q]] : -1;
        if (i >= 0 && i < m_local) {
          if (img_row) img_row[(int64_t)(s0 + q) * ld + t] = v[q];
          else A[(int64_t)i * ld + t] = v[q];
        }
      }
    }
  } else {  // b of every local row (LPState.java:164 / :146)
    const unsigned long long hit = __ballot((unsigned)(sh_l[lane] - t_wave) < 64u);
    const unsigned long long hit_hi = __ballot((unsigned)(sh_l[64 + lane] - t_wave) < 64u);
    if (t < m_local) {
      double bi = b_src[t];  // == b unless the sweep ran out of place
      for (int r0 = 0; r0 < np; r0 += 8) {
        double cv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) cv[q] = (r0 + q < np) ? col_ring[(int64_t)(r0 + q) * mp + t] : 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int r = r0 + q;
          if (r < np) {
            const double nb = submul(bi, cv[q], sh_bl[r]);
            bi = nb;
            if ((r < 64 ? hit >> r : hit_hi >> (r - 64)) & 1) { if (t == sh_l[r]) bi = sh_bl[r]; }
          }
        }
      }
      b[t] = bi;
    }
  }
}

// Behind the sweep of the overlapped loop: the entering columns (job 0) and pivot rows (job 1) that k_block_fixup computed
// beside it go from the images into the tableau.  grid = (ceil(max(m, ld)/256), ceil(K / 8), 2), the chains found as there.
__global__ __launch_bounds__(256) void k_block_fixup_scatter(double* __restrict__ A, int64_t ld, int m_local, int row0,
                                                             const double* __restrict__ img_col,
                                                             const double* __restrict__ img_row, int64_t mp,
                                                             const LpxCtl* __restrict__ ring, int kmax,
                                                             long long* __restrict__ clk) {
  if (clk && blockIdx.x < 8 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) {
    const unsigned x = xcc_id() & 7u;
    clk[x * 4 + 2] = __builtin_amdgcn_s_memtime(); clk[x * 4 + 3] = wall_clock64();
  }
  __shared__ int sh_key[kBlockMax], sh_pick[kBlockMax + kFixChunk];
  __shared__ int sh_np, sh_npick;
  const int s0 = blockIdx.y * kFixChunk, job = blockIdx.z;
  if ((int64_t)blockIdx.x * blockDim.x >= (job == 1 ? ld : (int64_t)m_local)) return;
  const int np = ring_count128(ring, kmax, &sh_np);
  if (s0 >= np) return;
  if ((int)threadIdx.x < kBlockMax) {
    const bool live = (int)threadIdx.x < np;
    const LpxCtl& q = ring[live ? threadIdx.x : 0];
    sh_key[threadIdx.x] = live ? (job == 1 ? q.l - row0 : q.e_cur) : -1;
  }
  __syncthreads();
  if (threadIdx.x < 64) fix_pick_chains(sh_key, np, sh_pick, &sh_npick);
  __syncthreads();
  const int npick = sh_npick;
  if (s0 >= npick) return;
  const int ns = min(kFixChunk, npick - s0);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  double v[kFixChunk];
  if (job == 0) {
    if (t >= m_local) return;
#pragma unroll
    for (int q = 0; q < kFixChunk; ++q) v[q] = q < ns ? img_col[(int64_t)(s0 + q) * mp + t] : 0.0;
#pragma unroll
    for (int q = 0; q < kFixChunk; ++q)
      if (q < ns) A[(int64_t)t * ld + sh_key[sh_pick[s0 + q]]] = v[q];
  } else {
    if (t >= (int)ld) return;
#pragma unroll
    for (int q = 0; q < kFixChunk; ++q) {
      const int i = q < ns ? sh_key[sh_pick[s0 + q]] : -1;
      v[q] = (i >= 0 && i < m_local) ? img_row[(int64_t)(s0 + q) * ld + t] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < kFixChunk; ++q) {
      const int i = q < ns ? sh_key[sh_pick[s0 + q]] : -1;
      if (i >= 0 && i < m_local) A[(int64_t)i * ld + t] = v[q];
    }
  }
}

