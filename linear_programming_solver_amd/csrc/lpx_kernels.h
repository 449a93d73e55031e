// Internal interface between the HIP kernels (lpx_kernels.hip) and the host engine (lpx_engine.cpp).
// Not part of the public ABI (that is include/lpx.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lpxk {

constexpr int kRunning = -1;     // LpxCtl::status while the loop is live; otherwise an lpx_status value
constexpr double kEps = 1e-9;    // DEF_EPSILON  reference LPState.java:20
constexpr double kInf = 1e50;    // DEF_INF      reference LPState.java:21

// (ratio, row) candidate of the minimum-ratio test; "none" is {kInf, INT32_MAX}.
struct RatioRow {
  double ratio;
  int32_t row;   // GLOBAL row index
  int32_t pad;
};

// Device-resident loop control: the host never decides anything per pivot, it only polls `status`.
struct LpxCtl {
  double v;            // objective constant (LPState.v)
  double p;            // pivot element A[l][e] of the pivot being applied
  double bl;           // b[l] / p
  double pc;           // c[e] before the pivot
  double ratio;        // winning ratio of the last ratio test
  int32_t e_next;      // entering slot chosen for the NEXT pivot (-1: none)
  int32_t e_cur;       // entering slot of the pivot being applied by k_update
  int32_t l;           // leaving row (GLOBAL index) of the pivot being applied / last ratio test winner
  int32_t status;      // kRunning or lpx_status
  int32_t do_update;   // 1 iff k_select_pivot performed a pivot that k_update must apply
  int32_t track;       // slot of the tracked variable (x0 in phase 1), -1 = none  (LPSolver.java:151-155)
  int32_t parity;      // col[parity] receives / holds column e_next
  int32_t e_min;       // scratch of the pivot-finish kernels: atomicMin target, INT32_MAX when idle
  int32_t ticket;      // scratch: arrival counter of the pivot-finish workgroups, 0 when idle
  int32_t reserved;
  int64_t pivots;      // pivots performed since lpx_simplex_loop started
  int64_t max_pivots;  // budget for `pivots` (<0: unlimited)
};

// What the first launch of a loop call resets in LpxCtl (k_entering / k_entering_dantzig): see loop_start().
struct LoopStart { int32_t reset = 0; int32_t track = -1; int64_t max_pivots = -1; };

struct Geometry {
  int U;              // double2 per thread per row in k_update (strip width = 512*U columns)
  int rows_per_tile;  // rows handled by one k_update block
  int nstrips, ntiles;
};

struct Buffers {
  double* A;          // m_local x ld, row-major, columns [n, ld) are zero
  int64_t ld;
  double* b;          // m_local
  double* c;          // ld (padding zero)
  double* prow;       // ld: normalised pivot row of the pivot being applied
  double* col[2];     // m_local each: column e of the tableau (ping-pong, see LpxCtl::parity)
  RatioRow* partial;  // ntiles
  int32_t* perm;      // n + m_global
  LpxCtl* ctl;
  int chain_form;     // decision kernel of the one-device blocked loop: 0 = k_block_chain_t, 1 = k_block_chain2_t (LPX_OPT_CHAIN_FORM)
  int fused;          // 0: lpxk::plain kernels (two roundings per update, the default); 1: lpxk::fused (LPX_OPT_FUSED)
};

// blocked pivoting: ring of pending pivots (see lpx_kernels.hip "blocked pivoting")
constexpr int kBlockMax = 128;       // pivots per block / slots per ring half (single-device loop)
constexpr int kShardBlockMax = 32;   // the step-wise shard interface and lpx_multi decide at most this many per block
constexpr int kChainMaxWgs = 256;   // <= one workgroup per CU: the whole grid is resident
constexpr int kMaxDevices = 8;      // row-block shards of one lpx_multi (the GPUs of one node)
struct BlockRing {  // every ring has 2 * kBlockMax slots: two halves, one per block in flight
  double* prow;   // kBlockMax x ld : normalised pivot row of pending pivot s
  double* col;    // kBlockMax x mp : column e_s of the tableau just before pivot s
  double* col0;   // kBlockMax x mp : the same column as it stands in the stale tableau (for the fix-up)
  double* row0;   // kBlockMax x ld : the stale pivot row l_s (for the fix-up)
  LpxCtl* up;     // kBlockMax parameter blocks (written by finish_pivot)
  int64_t mp;
  // scratch of k_block_chain (single-shard blocks decided in one persistent launch)
  void* chain_part_a;      // 2 x kChainMaxWgs x 32 B
  void* chain_part_b;      // kChainMaxWgs x 16 B
  unsigned* chain_bar;     // 2 barrier counters + the hand-off word, 128 B apart; a launch zeroes the next one's counter
  double* chain_own_col;   // kBlockMax x mp: copy of `col` that only its writer re-reads (plain, cache-resident)
  double* chain_own_prow;  // kBlockMax x ld: likewise for `prow`
  double* chain_own_dvc;   // kBlockMax x mp: column e_s of the tableau just AFTER pivot s (restart point)
  double* chain_own_b;     // mp: b with all pending pivots applied
  int32_t* chain_own_rs;   // mp + ld: k_block_chain2's start indices per row / per slot (last pending pivot that replaced it)
  long long* chain_dbg;    // diagnostics (LPX_OPT_CHAIN_TRACE): 5 timestamps per decision of the last block
  unsigned* census;        // [w] = XCC id + 1 of chain workgroup w; [kChainMaxWgs] = OR of (1 << XCC id) of sampled sweep workgroups
  double* fix_col;         // overlapped loop: images of the fix-up's entering columns [chain][mp] (NULL: the fix-up follows the sweep and writes the tableau itself)
  double* fix_row;         // ... and of its pivot rows [chain][ld]; both 2 x kBlockMax chains like the rings
  double* col_packed;      // k_sweep32_pull: the block's multipliers as [batch of 4 rows][pivot][row]: (mp / 4) x 1 KiB (2 KiB for blocks of 64, 4 KiB for k_sweep128_mfma: 16 KiB per 16-row tile)
  unsigned* tickets;       // k_sweep32_pull: one batch counter per 128-column sub-strip, 128 bytes apart (sweep_ticket_slots(ld) of them: k_sweep128_mfma takes one chunk counter and one per (64-column sub-strip, row range)); like col_packed once per ring half
  unsigned* sweep_fail;    // the word a pull kernel sets when a bounded wait ran out (k_sweep64_pull: variants library only)
  long long* clk;          // clock probe of the last pulled sweep, per XCD x: clk[4 x + 0..1] = {s_memtime, 100 MHz} in front of it, [4 x + 2..3] behind it
  const double* zeros;     // 256 bytes of +0.0: what k_sweep32_dma's multiplier DMA reads for the identity steps of a partly filled block
  // shards of an lpx_multi only (else NULL): written by the peers' decision kernels
  void* mg_mail;                   // MgMail[2][kMaxDevices]
  unsigned long long* mg_arrive;   // [kChainMaxWgs]
  double* mg_candrow;              // one-hop form: candidate rows [2][kMaxDevices][ld]
  unsigned long long* mg_arrive2;  // one-hop form: arrival words of the candidate rows [2][kMaxDevices][kChainMaxWgs]
};
// Row-block shards on several devices deciding together (lpx_multi): what a shard's launch needs to know about its
// peers.  Pointers are peer-mapped device pointers, index = shard rank; [dev] is the shard's own memory.
struct MgPeers {
  int n_dev, dev;
  int row0, m_global;
  int mail_slot0;                          // parity of the decisions taken by earlier launches of the loop
  void* mail[kMaxDevices];                 // MgMail[2][kMaxDevices] (32-byte records) of every shard
  double* prow[kMaxDevices];               // base of every shard's pivot-row ring (BlockRing::prow)
  unsigned long long* arrive[kMaxDevices]; // arrival words [kChainMaxWgs] of every shard
  int onehop;                              // 1: every shard ships its candidate's ROW with the candidate (one hop per decision)
  double* candrow[kMaxDevices];            // candidate rows [2][kMaxDevices][ld] of every shard
  unsigned long long* arrive2[kMaxDevices];// their arrival words [2][kMaxDevices][kChainMaxWgs]
  unsigned spin_max;                       // bound of the waits between devices in polls (0: the default, 2^22 = seconds)
};
// which kernel swept the bulk of the tableau (lpx_state_info.sweep_kernel)
enum SweepKernel { kSweepNone = 0, kSweepTiles = 1, kSweepMulti = 2, kSweepSteady = 3, kSweepPipe64 = 4, kSweepDma = 5, kSweepPull = 6, kSweepPull64 = 7, kSweepOne64 = 8, kSweepMfma64 = 9, kSweepMfma642 = 10, kSweepMfma128 = 11 };
// The fix-up of a block beside its sweep (launch_block_sweep): where its chains run and the two events that tie them in.
// ready: the block's decisions are through (the side stream waits for it); packed: the sweep's pack kernel is through (may be
// NULL: it then runs on the sweep's stream); done: the fix-up's chains are through (the copy kernel waits for it).
struct FixSide { hipStream_t stream; hipEvent_t ready, done, packed; };
constexpr int kColPackedRowBytes = 1024;   // BlockRing::col_packed per ring half: (mp / 4 + 1) batches of 4 x this many bytes
constexpr int kSweep128Ranges = 3;        // k_sweep128_mfma: row ranges per 64-column sub-strip (micro-benchmark at cfg4: 3 2.80 ms, 12 2.87, 32 2.97)
struct RestoreEntry { int32_t is_basic; int32_t index; double k; };  // index = row r (basic) or post-drop slot

// ---- batched solve (lpx_batch.inc / lpx_batch.cpp): many small LPs, one workgroup per LP, the whole state in LDS ----
// Image of ONE m x n LP, in doubles; the HBM copy and the front of the workgroup's LDS are the same image, so it moves
// in and out with 16-byte accesses:  A (m rows of pitch ld) | b[m] | c[n] | v | pad to even | perm int32[n + m] | pad to even.
// ld = n | 1: an odd pitch puts the m entries of a column on different LDS banks.  Behind the image the LDS holds what
// never leaves the chip: the saved entering column (m doubles, padded to even) and kBatchScratchBytes of reduction scratch.
constexpr int kBatchLdsMax = 163840;      // LPX_BATCH_LDS_BYTES: what gfx950 gives one workgroup
constexpr int kBatchScratchBytes = 512;   // 2 x 16 RatioRow: the per-wave partials of the entering and of the leaving reduction
struct BatchLayout {
  int64_t ld, b, c, v, perm, image, col;  // offsets in doubles (perm: of its first int32); image = doubles of the HBM image
  int64_t lds_bytes;
};
__host__ __device__ inline BatchLayout batch_layout(int64_t m, int64_t n) {
  BatchLayout L;
  L.ld = n | 1;
  L.b = m * L.ld;
  L.c = L.b + m;
  L.v = L.c + n;
  L.perm = (L.v + 2) & ~(int64_t)1;
  L.image = L.perm + (((n + m + 1) / 2 + 1) & ~(int64_t)1);
  L.col = L.image;
  L.lds_bytes = 8 * (L.image + ((m + 1) & ~(int64_t)1)) + kBatchScratchBytes;
  return L;
}
struct BatchArgs {
  int32_t count;
  const int32_t* m;        // [count]
  const int32_t* n;        // [count]
  const int64_t* offset;   // [count] first double of LP k's image in `image` (even)
  double* image;
  int64_t* pivots;         // [count] out: pivots of this call
  int32_t* status;         // [count] out: lpx_status
  int32_t* track;          // [count] in/out: tracked slot, -1 = none
  int64_t max_pivots;      // per LP; < 0: unlimited
  int32_t dantzig;
  int32_t fused;           // which compilation the dispatcher takes
  int32_t lds_bytes;       // dynamic LDS of the launch: the largest batch_layout(m, n).lds_bytes of the batch
  int32_t threads;         // workgroup size (multiple of 64, <= 1024)
};
// k_batch_solve (LPSolver.solve per workgroup): the LDS of an m x n LP that TAKES PHASE 1.  The workgroup then works in
// the image of the m x (n + 1) auxiliary LP (`aux`, with its saved column and reduction scratch) for the whole solve —
// after restoreInitialLP the tableau keeps the auxiliary pitch, one column narrower — and keeps behind it what
// restoreInitialLP needs: c0[n] (the form's c, negated for `min`), the restore order int32[n] and the slot of every
// original variable int32[n].  An LP that needs no phase 1 takes batch_layout(m, n) as in k_batch_simplex.
struct BatchSolveLayout {
  BatchLayout aux;
  int64_t c0, order, slot;   // offsets in doubles (order, slot: of their first int32)
  int64_t lds_bytes;
};
__host__ __device__ inline BatchSolveLayout batch_solve_layout(int64_t m, int64_t n) {
  BatchSolveLayout W;
  W.aux = batch_layout(m, n + 1);
  W.c0 = W.aux.lds_bytes / 8;
  W.order = W.c0 + ((n + 1) & ~(int64_t)1);
  W.slot = W.order + (n + 1) / 2;
  W.lds_bytes = 8 * (W.order + ((n + 1) & ~(int64_t)1));
  return W;
}
struct BatchSolveArgs {
  int32_t count;
  const int32_t* m;          // [count]
  const int32_t* n;          // [count] columns of the standard form
  const int64_t* offset;     // [count] first double of LP k's image; an LP with phase1[k] has room for batch_layout(m, n + 1)
  double* image;             // in: batch_layout(m, n); out: batch_layout(m, n_final)
  const int32_t* maximize;   // [count] or NULL: every LP is a maximisation
  const int32_t* phase1;     // [count] what the host found with minInB: it sized the image room and the LDS from it
  const int32_t* order;      // [count * order_pitch] restore order of LP k (original-variable indices)
  const int32_t* order_len;  // [count] its entries (<= n)
  int64_t order_pitch;
  int32_t* status;           // [count] out: lpx_status
  int32_t* phase1_used;      // [count] out
  int32_t* x0_slot;          // [count] out: -1 without phase 1
  int32_t* n_final;          // [count] out: n, or n + 1 when the solve ended inside phase 1
  int64_t* pivots1;          // [count] out
  int64_t* pivots2;          // [count] out
  double* v;                 // [count] out: the objective constant of the final state
  int64_t max_pivots;        // budget of the whole solve per LP; < 0: unlimited
  int32_t dantzig;
  int32_t fused;
  int32_t lds_bytes;
  int32_t threads;
};
// k_batch_scenarios (k_batch_solve for `count` scenarios of ONE constraint matrix): the matrix once, b and c as dense
// arrays, and no image in either direction.  The output fields carry the names they have in BatchSolveArgs: one body
// (batch_solve_body, lpx_batch.inc) writes both.
struct BatchScenarioArgs {
  int32_t count;
  int32_t m, n;              // every scenario's shape
  const double* A;           // m x n, row-major at pitch n: shared by every workgroup
  const double* b;           // scenario k's b[m] at b + k * ldb
  const double* c;           // scenario k's c[n] at c + k * ldc
  int64_t ldb, ldc;          // 0: one vector for every scenario
  const int32_t* flags;      // [count] bit 0: maximise; bit 1: the host's minInB found a negative b (it sized the LDS from it)
  const int32_t* order;      // [order_len] the ONE restore order (original-variable indices)
  int32_t order_len;         // <= n
  int32_t* status;           // [count] out: lpx_status
  int32_t* phase1_used;      // [count] out
  int32_t* x0_slot;          // [count] out: -1 without phase 1
  int32_t* n_final;          // [count] out: n, or n + 1 when the solve ended inside phase 1
  int64_t* pivots1;          // [count] out
  int64_t* pivots2;          // [count] out
  double* v;                 // [count] out: the objective constant of the final state
  double* x_out;             // [count * n] or NULL; row k written only when n_final[k] == n
  int32_t* perm_out;         // [count * (n + m)] or NULL; likewise
  int64_t max_pivots;        // budget of the whole solve per scenario; < 0: unlimited
  int32_t dantzig;
  int32_t fused;
  int32_t lds_bytes;
  int32_t threads;
};
// Re-solve from a shared basis (k_scenarios_crash, k_batch_resolve).  The crash kernel brings the handle's matrix to the
// basis ONCE and leaves an "eta file": per crash pivot t one entry of eta_stride(m, n) doubles
//   [0] entering slot e_t   [1] leaving row l_t   [2] pivot element piv_t   [3] 0
//   [4, 4 + m)          the entering column as batch_save_column saved it
//   [4 + m, 4 + m + n)  row l_t after the pivot (the normalised pivot row, entry e_t = 1/piv_t)
// which is all batch_pivot reads when it updates b, c and v: a scenario replays it in O(m + n) per entry.
__host__ __device__ inline int64_t eta_stride(int64_t m, int64_t n) { return m + n + 4; }
struct ScenarioCrashArgs {
  int32_t count;             // 1: one workgroup
  int32_t m, n;
  const double* A;           // m x n, row-major at pitch n
  const int32_t* wanted;     // [n + m] 1 where the variable id is to be basic
  double* A_out;             // m x n at pitch n: the matrix at the basis
  int32_t* perm_out;         // [n + m] the permutation at the basis
  double* eta;               // room for min(m, n) entries
  int32_t* info;             // [2] out: crash pivots made; the variable id at which the basis is singular, -1: none
  int32_t fused;
  int32_t lds_bytes;
  int32_t threads;
};
// BatchScenarioArgs with A = the matrix at the basis; of flags only bit 0 is read, order and order_len not at all, and
// the outputs of a scenario routed LPX_ROUTE_COLD (route[k] = 0) are left as they are.
struct BatchResolveArgs : BatchScenarioArgs {
  const int32_t* perm0;      // [n + m] the permutation at the basis
  const double* eta;
  int32_t n_eta;
  int32_t* route;            // [count] out: LPX_ROUTE_*
};

// ---- launch wrappers --------------------------------------------------------------------------------------------
// lpx_kernels.hip is compiled twice: plain (one rounding per reference operation) and fused (updates as one FMA).
namespace plain {
#include "lpx_launchers.inc"
}  // namespace plain
namespace fused {
#include "lpx_launchers.inc"
}  // namespace fused
// what the host engine calls: plain:: or fused:: by Buffers::fused (lpx_dispatch.cpp)
#include "lpx_launchers.inc"

}  // namespace lpxk
