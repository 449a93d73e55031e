// Batched solve behind the C ABI (include/lpx.h): many small LPs in ONE launch, one workgroup per LP with the LP's whole
// state in LDS (lpx_batch.inc: k_batch_simplex runs the loop, k_batch_solve the whole of LPSolver.solve with phase 1,
// k_batch_scenarios the same for many (b, c) on one matrix, k_scenarios_crash and k_batch_resolve the re-solve of such
// scenarios from a shared basis: lpx_scenarios at the end of this file).
// The handle keeps one HBM image per LP (lpxk::BatchLayout).  Every piece of the host path exists once: Forms,
// check_one_shot, Gathered, solve_alone and stamp_seconds for the two batch one-shots; SolveScalars (the seven scalars a
// kernel answers per LP) for the three solves; launch_scenarios, download_rows and with_scenarios for the scenario calls;
// one LaunchShape for a launch and the lpxi_*_launch_info that describes it; DeviceBuf members own the device memory.
// Every argument is checked before the first device call: a bad call answers LPX_BAD_ARGUMENT without a GPU too.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "lpx_internal.h"

namespace lpx_internal {
void round6_text(double v, char* out, size_t cap);   // lpx_solver.cpp
}

namespace {

double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// A device array that frees itself.  The device it was allocated on must be current when it goes: the destructors of the
// two handles below see to that.
template <class T>
class DeviceBuf {
 public:
  DeviceBuf() = default;
  DeviceBuf(DeviceBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }   // move-only: no copy, no assignment
  ~DeviceBuf() { reset(); }
  hipError_t alloc(size_t n) {   // room for n entries; what it held before is freed first
    reset();
    return hipMalloc((void**)&p_, n * sizeof(T));
  }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
  }
  T* get() const { return p_; }

 private:
  T* p_ = nullptr;
};

void fill_objective(lpx_solve_result& r, double v, bool maximize) {
  if (!maximize) v = -v;                                                            // LPSolver.java:90
  r.objective = v;
  lpx_internal::round6_text(v, r.objective_text, sizeof r.objective_text);         // :113
  r.objective_rounded = strtod(r.objective_text, nullptr);
}

// The seven scalars a solve kernel answers per LP -- status, phase1_used, x0_slot, n_final (int32), pivots1, pivots2
// (int64) and v -- as three device arrays of 4, 2 and 1 entries per LP, and their host copies.
struct SolveScalars {
  int reserve(size_t count) {
    HIP_TRY(d_i32.alloc(4 * count));
    HIP_TRY(d_i64.alloc(2 * count));
    HIP_TRY(d_v.alloc(count));
    return 0;
  }
  // the seven output fields of a BatchSolveArgs, BatchScenarioArgs or BatchResolveArgs for a launch of `count` LPs
  template <class Args>
  void bind(Args& a, int32_t count) {
    cnt = (size_t)count;
    a.status = d_i32.get();
    a.phase1_used = a.status + cnt;
    a.x0_slot = a.status + 2 * cnt;
    a.n_final = a.status + 3 * cnt;
    a.pivots1 = d_i64.get();
    a.pivots2 = a.pivots1 + cnt;
    a.v = d_v.get();
    h_i32.resize(4 * cnt);
    h_i64.resize(2 * cnt);
    h_v.resize(cnt);
  }
  // what the launch wrote, on the host when this returns
  int fetch(hipStream_t stream) {
    HIP_TRY(hipMemcpyAsync(h_i32.data(), d_i32.get(), h_i32.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(h_i64.data(), d_i64.get(), h_i64.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(h_v.data(), d_v.get(), h_v.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
  }
  int32_t n_final(int32_t k) const { return h_i32[3 * cnt + k]; }
  // LP k's scalars into r (the times are the caller's); true: the kernel reported LPX_DEVICE_ERROR
  bool decode(int32_t k, bool maximize, lpx_solve_result& r) const {
    r.status = h_i32[k];
    r.phase1_used = h_i32[cnt + k];
    r.x0_slot = h_i32[2 * cnt + k];
    r.pivots_phase1 = h_i64[k];
    r.pivots_phase2 = h_i64[cnt + k];
    fill_objective(r, h_v[k], maximize);
    return r.status == LPX_DEVICE_ERROR;
  }

 private:
  DeviceBuf<int32_t> d_i32;
  DeviceBuf<int64_t> d_i64;
  DeviceBuf<double> d_v;
  std::vector<int32_t> h_i32;
  std::vector<int64_t> h_i64;
  std::vector<double> h_v;
  size_t cnt = 0;   // LPs of the launch bound last
};

}  // namespace

struct lpx_batch {
  int device = 0;
  int32_t count = 0, m_max = 0, n_max = 0;
  std::vector<int32_t> m, n;
  std::vector<int64_t> offset;      // first double of LP k's image; offset[count] = doubles of all images
  int32_t lds_bytes = 0;            // dynamic LDS of the launch: the largest LP's
  int32_t threads = 64;             // workgroup size chosen for the batch
  int fused = 0, pricing = 0;
  hipStream_t stream = nullptr;
  DeviceBuf<double> d_image;
  DeviceBuf<int64_t> d_offset, d_pivots;
  DeviceBuf<int32_t> d_m, d_n, d_status, d_track;
  // lpx_batch_solve
  std::vector<int32_t> n_cur;       // columns of LP k now: n[k], or n[k] + 1 after a solve that ended inside phase 1
  std::vector<int32_t> need_p1;     // minInB of the b given at creation finds a negative entry: the image has room for n + 1 columns
  bool custom_start = false;        // created with a nonzero v or with perm: not the start of LPSolver.solve
  int state = 0;                    // 0: as created, 1: a loop has run, 2: solved
  int32_t solve_threads = 64;       // workgroup size of k_batch_solve: by the auxiliary shape where phase 1 is due
  // inputs and outputs of k_batch_solve, allocated with the handle: flags, orders, the seven scalars per LP
  DeviceBuf<int32_t> d_max, d_p1, d_order, d_olen;
  SolveScalars scalars;

  // nothing is allocated before the stream exists; the members free themselves after this body
  ~lpx_batch() {
    if (!stream) return;
    (void)hipSetDevice(device);
    (void)hipStreamDestroy(stream);
  }
};

namespace {

int64_t solve_lds_bytes_of(int64_t m, int64_t n) {
  if (m < 0 || n < 0) return -1;
  if ((double)m * (double)((n + 1) | 1) > 1e12) return INT64_MAX;
  return lpxk::batch_solve_layout(m, n).lds_bytes;
}

int64_t lds_bytes_of(int64_t m, int64_t n) {
  if (m < 0 || n < 0) return -1;
  if ((double)m * (double)(n | 1) > 1e12) return INT64_MAX;   // far beyond any LDS; keeps the formula inside int64
  return lpxk::batch_layout(m, n).lds_bytes;
}

// `count` LPs inside m_max x n_max as the ABI passes them: shapes (NULL: all m_max x n_max), A with row pitch lda and
// strideA between LPs, b and c at the pitches m_max and n_max, and for the one-shot calls the `max` flags (NULL: all max)
struct Forms {
  int32_t count, m_max, n_max;
  const int32_t *m, *n;
  const double* A;
  int64_t lda, strideA;
  const double *b, *c;
  const int32_t* maximize;
  int32_t rows(int32_t k) const { return m ? m[k] : m_max; }
  int32_t cols(int32_t k) const { return n ? n[k] : n_max; }
  const double* A_of(int32_t k) const { return A ? A + (int64_t)k * strideA : nullptr; }
  const double* b_of(int32_t k) const { return b ? b + (int64_t)k * m_max : nullptr; }
  const double* c_of(int32_t k) const { return c ? c + (int64_t)k * n_max : nullptr; }
  bool maximizes(int32_t k) const { return !maximize || maximize[k] != 0; }
  // minInB (LPSolver.java:375-386) finds an entry below 0 in LP k's b: the form needs the auxiliary LP (:119)
  bool phase1(int32_t k) const {
    const double* bk = b_of(k);
    double mn = 1e50;
    int idx = -1;
    for (int i = 0; i < rows(k); i++)
      if (mn > bk[i]) { mn = bk[i]; idx = i; }
    return !(idx == -1 || bk[idx] >= 0.0);
  }
};

// Workgroup size of one LP: a wave per 64-column chunk times up to four row groups of at least 16 rows, at most 16
// waves.  One wave (no workgroup barriers) up to 16 x 64; 256 threads for 64 x 64; 1024 from 64 x 256 or 49 x 200 on.
int threads_of(int32_t m, int32_t n) {
  const int nq = std::max(1, (n + 63) / 64);
  const int groups = std::min(4, std::max(1, (m + 15) / 16));
  return 64 * std::min(16, nq * groups);
}

// shapes of a batch: every LP inside m_max x n_max and inside the LDS of one workgroup; then the arrays those shapes read
int check_forms(const char* who, const Forms& F) {
  if (F.count < 0 || F.m_max < 0 || F.n_max < 0)
    return fail(LPX_BAD_ARGUMENT, std::string(who) + ": negative count or dimension");
  if ((F.m == nullptr) != (F.n == nullptr)) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": m and n must both be given or both be NULL");
  for (int32_t k = 0; k < F.count; k++) {
    const int32_t mk = F.rows(k), nk = F.cols(k);
    char msg[200];
    if (mk < 0 || nk < 0 || mk > F.m_max || nk > F.n_max) {
      snprintf(msg, sizeof msg, "%s: LP %d has shape %d x %d outside 0..%d x 0..%d", who, k, mk, nk, F.m_max, F.n_max);
      return fail(LPX_BAD_ARGUMENT, msg);
    }
    const int64_t need = lds_bytes_of(mk, nk);
    if (need > LPX_BATCH_LDS_BYTES) {
      snprintf(msg, sizeof msg, "%s: LP %d of shape %d x %d needs %lld bytes of LDS, a workgroup has %d", who, k, mk, nk,
               (long long)need, LPX_BATCH_LDS_BYTES);
      return fail(LPX_BAD_ARGUMENT, msg);
    }
  }
  bool needA = false, needb = false, needc = false;
  for (int32_t k = 0; k < F.count; k++) {
    needA |= F.rows(k) > 0 && F.cols(k) > 0;
    needb |= F.rows(k) > 0;
    needc |= F.cols(k) > 0;
  }
  if (F.lda < F.n_max || F.strideA < 0) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": lda < n_max or negative strideA");
  if ((needA && !F.A) || (needb && !F.b) || (needc && !F.c)) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": NULL array where data is due");
  return 0;
}

using BatchGuard = std::unique_ptr<lpx_batch>;

// the checked core of lpx_batch_create (no argument checks: the callers have made them); a failure leaves `out` empty
// and nothing allocated
int create_checked(const Forms& F, const double* v, const int32_t* perm, int device, BatchGuard& out) {
  const int32_t count = F.count, m_max = F.m_max, n_max = F.n_max;
  BatchGuard guard(new lpx_batch());
  lpx_batch* B = guard.get();
  B->device = device;
  B->count = count;
  B->m_max = m_max;
  B->n_max = n_max;
  B->m.resize(count);
  B->n.resize(count);
  B->offset.resize((size_t)count + 1);
  B->need_p1.resize(count);
  B->custom_start = perm != nullptr;
  for (int32_t k = 0; v && k < count; k++) B->custom_start |= !(v[k] == 0.0);
  int64_t total = 0, lds = 0;
  int threads = 64, solve_threads = 64;
  for (int32_t k = 0; k < count; k++) {
    B->m[k] = F.rows(k);
    B->n[k] = F.cols(k);
    const lpxk::BatchLayout L = lpxk::batch_layout(B->m[k], B->n[k]);
    B->need_p1[k] = F.phase1(k);
    B->offset[k] = total;
    // a form that needs phase 1 may come back from lpx_batch_solve as its m x (n + 1) auxiliary LP
    total += B->need_p1[k] ? std::max(L.image, lpxk::batch_layout(B->m[k], B->n[k] + 1).image) : L.image;
    lds = std::max(lds, L.lds_bytes);
    threads = std::max(threads, threads_of(B->m[k], B->n[k]));
    solve_threads = std::max(solve_threads, threads_of(B->m[k], B->n[k] + (B->need_p1[k] ? 1 : 0)));
  }
  B->n_cur = B->n;
  B->offset[count] = total;
  B->lds_bytes = (int32_t)lds;
  B->threads = threads;
  B->solve_threads = solve_threads;
  std::vector<double> img((size_t)total, 0.0);
  for (int32_t k = 0; k < count; k++) {
    const int32_t mk = B->m[k], nk = B->n[k];
    const lpxk::BatchLayout L = lpxk::batch_layout(mk, nk);
    double* g = img.data() + B->offset[k];
    for (int32_t i = 0; i < mk; i++)
      if (nk > 0) memcpy(g + (int64_t)i * L.ld, F.A_of(k) + (int64_t)i * F.lda, (size_t)nk * sizeof(double));
    if (mk > 0) memcpy(g + L.b, F.b_of(k), (size_t)mk * sizeof(double));
    if (nk > 0) memcpy(g + L.c, F.c_of(k), (size_t)nk * sizeof(double));
    g[L.v] = v ? v[k] : 0.0;
    int32_t* p = (int32_t*)(g + L.perm);
    for (int32_t s = 0; s < nk + mk; s++) p[s] = perm ? perm[(int64_t)k * ((int64_t)n_max + m_max) + s] : s;
  }
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreateWithFlags(&B->stream, hipStreamNonBlocking));
  const size_t cnt = (size_t)std::max(count, 1);
  HIP_TRY(B->d_image.alloc(std::max<size_t>((size_t)total, 2)));
  HIP_TRY(B->d_offset.alloc(cnt));
  HIP_TRY(B->d_pivots.alloc(cnt));
  HIP_TRY(B->d_m.alloc(cnt));
  HIP_TRY(B->d_n.alloc(cnt));
  HIP_TRY(B->d_status.alloc(cnt));
  HIP_TRY(B->d_track.alloc(cnt));
  HIP_TRY(B->d_max.alloc(cnt));
  HIP_TRY(B->d_p1.alloc(cnt));
  HIP_TRY(B->d_order.alloc(cnt * (size_t)std::max(n_max, 1)));
  HIP_TRY(B->d_olen.alloc(cnt));
  if (int rc = B->scalars.reserve(cnt)) return rc;
  if (total > 0) HIP_TRY(hipMemcpyAsync(B->d_image.get(), img.data(), (size_t)total * sizeof(double), hipMemcpyHostToDevice, B->stream));
  if (count > 0) {
    HIP_TRY(hipMemcpyAsync(B->d_offset.get(), B->offset.data(), (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice, B->stream));
    HIP_TRY(hipMemcpyAsync(B->d_m.get(), B->m.data(), (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, B->stream));
    HIP_TRY(hipMemcpyAsync(B->d_n.get(), B->n.data(), (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, B->stream));
    HIP_TRY(hipMemcpyAsync(B->d_p1.get(), B->need_p1.data(), (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, B->stream));
  }
  HIP_TRY(hipStreamSynchronize(B->stream));   // img goes out of scope
  out = std::move(guard);
  return 0;
}

// what a launch asks for; the launch itself and the lpxi_*_launch_info call that describes it read the same one
struct LaunchShape {
  int threads;
  int64_t lds_bytes;
};

// LPX_BATCH_THREADS (debugging aid of scripts/bench_batch.py, read at every loop call): workgroup size instead of the
// by-size choice, rounded down to a multiple of 64 inside 64..1024
int threads_or_env(int by_size) {
  const char* e = getenv("LPX_BATCH_THREADS");
  if (e && *e) {
    const int t = atoi(e);
    if (t > 0) return std::max(64, std::min(1024, t / 64 * 64));
  }
  return by_size;
}

int threads_in_effect(const lpx_batch* B, bool solve = false) { return threads_or_env(solve ? B->solve_threads : B->threads); }

// dynamic LDS of the k_batch_solve launch: per LP the auxiliary layout where phase 1 is due, else the plain one
int64_t solve_launch_lds(const lpx_batch* B) {
  int64_t lds = lpxk::kBatchScratchBytes;
  for (int32_t k = 0; k < B->count; k++)
    lds = std::max(lds, B->need_p1[k] ? solve_lds_bytes_of(B->m[k], B->n[k]) : lds_bytes_of(B->m[k], B->n[k]));
  return lds;
}

// the launch of lpx_batch_simplex_loop (k_batch_simplex) or of lpx_batch_solve (k_batch_solve) on this handle
LaunchShape batch_shape(const lpx_batch* B, bool solve) {
  return {threads_in_effect(B, solve), solve ? solve_launch_lds(B) : B->lds_bytes};
}

// the launch of a kernel that gives one workgroup an m x n LP of a scenario batch: k_batch_scenarios (phase1: some
// scenario needs the auxiliary LP, and every workgroup gets its room), k_scenarios_crash and k_batch_resolve (never)
LaunchShape scenario_shape(int32_t m, int32_t n, bool phase1) {
  return {threads_or_env(threads_of(m, n + (phase1 ? 1 : 0))),
          std::max<int64_t>(lpxk::kBatchScratchBytes, phase1 ? solve_lds_bytes_of(m, n) : lds_bytes_of(m, n))};
}

// threads, LDS bytes and resident workgroups per CU (`occupancy` of the kernel in question) of a launch, into the
// pointers of an lpxi_*_launch_info call that are not NULL
template <class Occupancy>
int report_launch(int device, LaunchShape shape, Occupancy occupancy, int32_t* threads, int32_t* lds_bytes, int32_t* blocks_per_cu) {
  DeviceRestore keep_device;
  HIP_TRY(hipSetDevice(device));
  const int lds = (int)std::min<int64_t>(shape.lds_bytes, INT32_MAX);
  if (threads) *threads = shape.threads;
  if (lds_bytes) *lds_bytes = lds;
  if (blocks_per_cu) *blocks_per_cu = occupancy(shape.threads, lds);
  return 0;
}

// one restore order of `len` entries (< 0: n) against an LP with n columns
int check_order(const char* who, int32_t k, int32_t m, int32_t n, const int32_t* order, int32_t len) {
  char msg[200];
  if (len < 0) len = n;
  if (len > n) {
    snprintf(msg, sizeof msg, "%s: restore order of LP %d (%d x %d) has %d entries", who, k, m, n, len);
    return fail(LPX_BAD_ARGUMENT, msg);
  }
  for (int32_t t = 0; t < len; t++)
    if (order[t] < 0 || order[t] >= n) {
      snprintf(msg, sizeof msg, "%s: restore order of LP %d (%d x %d) names variable %d at entry %d", who, k, m, n, order[t], t);
      return fail(LPX_BAD_ARGUMENT, msg);
    }
  return 0;
}

int too_large_for_phase1(const char* who, int32_t k, int32_t m, int32_t n) {
  char msg[240];
  snprintf(msg, sizeof msg, "%s: LP %d of shape %d x %d needs phase 1 and with it %lld bytes of LDS, a workgroup has %d", who, k,
           m, n, (long long)solve_lds_bytes_of(m, n), LPX_BATCH_LDS_BYTES);
  return fail(LPX_BAD_ARGUMENT, msg);
}

void init_results(lpx_solve_result* results, int32_t count) {
  for (int32_t k = 0; k < count; k++) {
    memset(&results[k], 0, sizeof results[k]);
    results[k].x0_slot = -1;
    results[k].status = LPX_BAD_ARGUMENT;
  }
}

// the times of a call that began at t_start: the same in every result
void stamp_seconds(lpx_solve_result* results, int32_t count, double t_start, double t_pivots) {
  const double t_total = now_s() - t_start;
  for (int32_t k = 0; k < count; k++) {
    results[k].seconds_total = t_total;
    results[k].seconds_pivots = t_pivots;
  }
}

// every LP's image from ONE copy through the handle's stream
int read_images(const lpx_batch* B, std::vector<double>& img) {
  img.resize((size_t)B->offset[B->count]);
  if (img.empty()) return 0;
  HIP_TRY(hipSetDevice(B->device));
  HIP_TRY(hipMemcpyAsync(img.data(), B->d_image.get(), img.size() * sizeof(double), hipMemcpyDeviceToHost, B->stream));
  HIP_TRY(hipStreamSynchronize(B->stream));
  return 0;
}

// x and perm of LP t of the handle, from the images read back, into row k of x_out and perm_out (either may be NULL); the
// auxiliary LP of a solve that ended inside phase 1 does not hold the caller's variables: its rows stay as they are
void write_solution(const lpx_batch* B, const std::vector<double>& img, int32_t t, int32_t k, double* x_out, int32_t* perm_out) {
  const int32_t mt = B->m[t], nt = B->n[t];
  if (B->n_cur[t] != nt) return;
  const lpxk::BatchLayout L = lpxk::batch_layout(mt, nt);
  const double* g = img.data() + B->offset[t];
  const int32_t* fp = (const int32_t*)(g + L.perm);
  if (perm_out && nt + mt > 0) memcpy(perm_out + k * ((int64_t)B->n_max + B->m_max), fp, ((size_t)nt + mt) * sizeof(int32_t));
  if (!x_out) return;
  double* x = x_out + (int64_t)k * B->n_max;
  for (int32_t j = 0; j < nt; j++) x[j] = 0.0;
  for (int32_t i = 0; i < mt; i++) {
    const int32_t id = fp[(size_t)nt + i];
    if (id >= 0 && id < nt) x[id] = g[L.b + i];
  }
}

int launch_info(const char* who, lpx_batch* B, bool solve, int32_t* threads, int32_t* lds_bytes, int32_t* blocks_per_cu) {
  if (!B) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": NULL handle");
  const auto occupancy = solve ? lpxk::batch_solve_blocks_per_cu : lpxk::batch_blocks_per_cu;
  return report_launch(B->device, batch_shape(B, solve), occupancy, threads, lds_bytes, blocks_per_cu);
}

// The options of a one-shot call into `o` (NULL: the defaults) without what a batch cannot honour; `field` is how `who`
// names those.  device_too: a negative device is refused here, beside a bad pricing, and the message says so (the
// scenario calls refuse it with the matrix, in words of their own).
int take_options(const char* who, const char* field, bool device_too, const lpx_solve_options* opts, lpx_solve_options& o) {
  o = lpx_solve_options{};
  o.max_pivots = -1;
  if (opts) o = *opts;
  const std::string f(field);
  if (o.keep_state || o.perm_out || o.x_out)
    return fail(LPX_BAD_ARGUMENT, std::string(who) + ": " + f + "keep_state, " + f + "perm_out and " + f + "x_out must be NULL");
  if ((device_too && o.device < 0) || (o.pricing != 0 && o.pricing != 1))
    return fail(LPX_BAD_ARGUMENT, std::string(who) + (device_too ? ": bad device or pricing" : ": bad pricing"));
  return 0;
}

// The argument checks of a one-shot batch call in their order: shapes, arrays, results (and the flags where
// maximize_due), then the options (take_options).
int check_one_shot(const char* who, const Forms& F, bool maximize_due, const lpx_solve_result* results, const char* field,
                   const lpx_solve_options* opts, lpx_solve_options& o) {
  if (int rc = check_forms(who, F)) return rc;
  if (F.count > 0 && (!results || (maximize_due && !F.maximize)))
    return fail(LPX_BAD_ARGUMENT, std::string(who) + (maximize_due ? ": results or maximize is NULL" : ": results is NULL"));
  return take_options(who, field, true, opts, o);
}

// The forms `index` names, gathered into dense arrays of their own (G): A rows copied from where they are, b and c as
// they are -- but negate_c_for_min: c0 = -c for a `min` form (LPSolver.java:86-89) on the host, for the kernel that knows no `min`
struct Gathered {
  std::vector<int32_t> m, n;
  std::vector<double> A, b, c;
  Forms G;
  Gathered(const Gathered&) = delete;   // G points into the vectors

  Gathered(const Forms& F, const std::vector<int32_t>& index, bool negate_c_for_min) : m(index.size()), n(index.size()) {
    const size_t nb = index.size(), ldp = std::max(F.n_max, 1), strideP = F.m_max * ldp;
    A.assign(nb * strideP, 0.0);
    b.assign(nb * F.m_max, 0.0);
    c.assign(nb * F.n_max, 0.0);
    for (size_t t = 0; t < nb; t++) {
      const int32_t k = index[t];
      m[t] = F.rows(k);
      n[t] = F.cols(k);
      const bool negate = negate_c_for_min && !F.maximizes(k);
      for (int32_t i = 0; i < m[t]; i++) {
        if (n[t] > 0) memcpy(&A[t * strideP + i * ldp], F.A_of(k) + (int64_t)i * F.lda, (size_t)n[t] * sizeof(double));
        b[t * F.m_max + i] = F.b_of(k)[i];
      }
      for (int32_t j = 0; j < n[t]; j++) c[t * F.n_max + j] = negate ? -F.c_of(k)[j] : F.c_of(k)[j];
    }
    G = Forms{(int32_t)nb, F.m_max, F.n_max, m.data(), n.data(), A.data(), (int64_t)ldp, (int64_t)strideP, b.data(), c.data(), nullptr};
  }

  // the handle of the gathered forms, owned by `guard`
  int create(const lpx_solve_options& o, BatchGuard& guard) const {
    if (int rc = create_checked(G, nullptr, nullptr, o.device, guard)) return rc;
    guard->fused = o.fused > 0;   // 0 = the library's choice by size = two roundings here, as in lpx_solve at these sizes
    guard->pricing = o.pricing;
    return 0;
  }
};

// lpx_solve for the forms left out of the batch, into their results and their rows of x_out / perm_out (NULL: none)
int solve_alone(const Forms& F, const std::vector<int32_t>& alone, const lpx_solve_options& o, lpx_solve_result* results,
                double* x_out, int32_t* perm_out, double& t_pivots) {
  const int64_t pw = (int64_t)F.n_max + F.m_max;
  for (int32_t k : alone) {
    lpx_solve_options oa = o;
    oa.x_out = x_out ? x_out + (int64_t)k * F.n_max : nullptr;
    oa.perm_out = perm_out ? perm_out + k * pw : nullptr;
    const int rc = lpx_solve(F.rows(k), F.cols(k), F.A_of(k), F.lda, F.b_of(k), F.c_of(k), F.maximizes(k), &oa, &results[k]);
    if (rc == LPX_DEVICE_ERROR || rc == LPX_BAD_ARGUMENT) return rc;
    t_pivots += results[k].seconds_pivots;
  }
  return 0;
}

}  // namespace

extern "C" int64_t lpx_batch_lds_bytes(int32_t m, int32_t n) {
  const int64_t r = lds_bytes_of(m, n);
  if (r < 0) fail(LPX_BAD_ARGUMENT, "lpx_batch_lds_bytes: negative dimension");
  return r;
}

extern "C" int64_t lpx_batch_solve_lds_bytes(int32_t m, int32_t n) {
  const int64_t r = solve_lds_bytes_of(m, n);
  if (r < 0) fail(LPX_BAD_ARGUMENT, "lpx_batch_solve_lds_bytes: negative dimension");
  return r;
}

extern "C" int lpx_batch_create(int32_t count, int32_t m_max, int32_t n_max, const int32_t* m, const int32_t* n,
                                const double* A, int64_t lda, int64_t strideA, const double* b, const double* c,
                                const double* v, const int32_t* perm, int device, lpx_batch** out) {
  if (!out) return fail(LPX_BAD_ARGUMENT, "lpx_batch_create: out is NULL");
  *out = nullptr;
  const Forms F{count, m_max, n_max, m, n, A, lda, strideA, b, c, nullptr};
  if (int rc = check_forms("lpx_batch_create", F)) return rc;
  if (device < 0) return fail(LPX_BAD_ARGUMENT, "lpx_batch_create: negative device");
  DeviceRestore keep_device;
  BatchGuard B;
  const int rc = create_checked(F, v, perm, device, B);
  *out = B.release();
  return rc;
}

extern "C" void lpx_batch_destroy(lpx_batch* B) {
  DeviceRestore keep_device;
  delete B;
}

extern "C" int lpx_batch_count(const lpx_batch* B) { return B ? B->count : 0; }

extern "C" int lpx_batch_set_option(lpx_batch* B, int32_t key, int64_t value) {
  if (!B) return fail(LPX_BAD_ARGUMENT, "lpx_batch_set_option: NULL handle");
  if (key != LPX_OPT_FUSED || value < 0 || value > 2)
    return fail(LPX_BAD_ARGUMENT, "lpx_batch_set_option: only LPX_OPT_FUSED (0, 1, 2) applies to a batch");
  B->fused = value == 1;   // 2 = by size: every LP of a batch is far below the switch, i.e. 0
  return 0;
}

extern "C" int lpx_batch_set_pricing(lpx_batch* B, int32_t pricing) {
  if (!B || (pricing != 0 && pricing != 1)) return fail(LPX_BAD_ARGUMENT, "lpx_batch_set_pricing: bad argument");
  B->pricing = pricing;
  return 0;
}

extern "C" int lpx_batch_simplex_loop(lpx_batch* B, int64_t max_pivots, int64_t* pivots_done, int32_t* status,
                                      int32_t* track_slot) {
  if (!B) return fail(LPX_BAD_ARGUMENT, "lpx_batch_simplex_loop: NULL handle");
  if (B->count > 0 && (!pivots_done || !status)) return fail(LPX_BAD_ARGUMENT, "lpx_batch_simplex_loop: NULL output array");
  if (B->state == 2) return fail(LPX_BAD_ARGUMENT, "lpx_batch_simplex_loop: the batch has been solved (lpx_batch_solve)");
  if (B->count == 0) return 0;
  if (track_slot)
    for (int32_t k = 0; k < B->count; k++)
      if (track_slot[k] < -1 || track_slot[k] >= B->n[k] + B->m[k])
        return fail(LPX_BAD_ARGUMENT, "lpx_batch_simplex_loop: tracked slot " + std::to_string(track_slot[k]) + " of LP " +
                                          std::to_string(k) + " is outside its n + m slots");
  DeviceRestore keep_device;
  HIP_TRY(hipSetDevice(B->device));
  B->state = 1;
  const size_t cnt = (size_t)B->count;
  if (track_slot) HIP_TRY(hipMemcpyAsync(B->d_track.get(), track_slot, cnt * sizeof(int32_t), hipMemcpyHostToDevice, B->stream));
  else HIP_TRY(hipMemsetAsync(B->d_track.get(), 0xff, cnt * sizeof(int32_t), B->stream));   // -1: nothing tracked
  const LaunchShape shape = batch_shape(B, false);
  lpxk::BatchArgs a{};
  a.count = B->count;
  a.m = B->d_m.get();
  a.n = B->d_n.get();
  a.offset = B->d_offset.get();
  a.image = B->d_image.get();
  a.pivots = B->d_pivots.get();
  a.status = B->d_status.get();
  a.track = B->d_track.get();
  a.max_pivots = max_pivots;
  a.dantzig = B->pricing == 1;
  a.fused = B->fused;
  a.lds_bytes = (int32_t)shape.lds_bytes;
  a.threads = shape.threads;
  HIP_TRY(lpxk::launch_batch_simplex(a, B->stream));
  HIP_TRY(hipMemcpyAsync(pivots_done, B->d_pivots.get(), cnt * sizeof(int64_t), hipMemcpyDeviceToHost, B->stream));
  HIP_TRY(hipMemcpyAsync(status, B->d_status.get(), cnt * sizeof(int32_t), hipMemcpyDeviceToHost, B->stream));
  if (track_slot) HIP_TRY(hipMemcpyAsync(track_slot, B->d_track.get(), cnt * sizeof(int32_t), hipMemcpyDeviceToHost, B->stream));
  HIP_TRY(hipStreamSynchronize(B->stream));
  return 0;
}

extern "C" int lpx_batch_read(lpx_batch* B, int32_t index, double* A, int64_t lda, double* b, double* c, double* v,
                              int32_t* perm) {
  if (!B || index < 0 || index >= B->count) return fail(LPX_BAD_ARGUMENT, "lpx_batch_read: bad handle or index");
  const int32_t mk = B->m[index], nk = B->n_cur[index];
  if (A && lda < nk) return fail(LPX_BAD_ARGUMENT, "lpx_batch_read: lda < n");
  const lpxk::BatchLayout L = lpxk::batch_layout(mk, nk);
  std::vector<double> img((size_t)L.image);
  DeviceRestore keep_device;
  HIP_TRY(hipSetDevice(B->device));
  HIP_TRY(hipMemcpyAsync(img.data(), B->d_image.get() + B->offset[index], img.size() * sizeof(double), hipMemcpyDeviceToHost, B->stream));
  HIP_TRY(hipStreamSynchronize(B->stream));
  if (A && nk > 0)
    for (int32_t i = 0; i < mk; i++) memcpy(A + (int64_t)i * lda, img.data() + (int64_t)i * L.ld, (size_t)nk * sizeof(double));
  if (b && mk > 0) memcpy(b, img.data() + L.b, (size_t)mk * sizeof(double));
  if (c && nk > 0) memcpy(c, img.data() + L.c, (size_t)nk * sizeof(double));
  if (v) *v = img[L.v];
  if (perm && nk + mk > 0) memcpy(perm, img.data() + L.perm, ((size_t)nk + mk) * sizeof(int32_t));
  return 0;
}

extern "C" int lpx_batch_shape(const lpx_batch* B, int32_t index, int32_t* m, int32_t* n) {
  if (!B || index < 0 || index >= B->count) return fail(LPX_BAD_ARGUMENT, "lpx_batch_shape: bad handle or index");
  if (m) *m = B->m[index];
  if (n) *n = B->n_cur[index];
  return 0;
}

// LPSolver.solve (LPSolver.java:78) for every LP of the handle in ONE launch of k_batch_solve: phase 1 included.
extern "C" int lpx_batch_solve(lpx_batch* B, const int32_t* maximize, int64_t max_pivots, const int32_t* restore_order,
                               const int32_t* restore_order_len, lpx_solve_result* results) {
  if (!B) return fail(LPX_BAD_ARGUMENT, "lpx_batch_solve: NULL handle");
  if (B->state != 0) return fail(LPX_BAD_ARGUMENT, "lpx_batch_solve: a loop or a solve has already run on this handle");
  if (B->custom_start) return fail(LPX_BAD_ARGUMENT, "lpx_batch_solve: the handle was created with a nonzero v or with perm, not from standard forms");
  const int32_t count = B->count;
  if (count > 0 && !results) return fail(LPX_BAD_ARGUMENT, "lpx_batch_solve: results is NULL");
  if (count == 0) return 0;
  const double t_start = now_s();
  const int64_t pitch = std::max(B->n_max, 1);
  std::vector<int32_t> order((size_t)count * pitch, 0), olen(count, 0);
  for (int32_t k = 0; k < count; k++) {
    if (!B->need_p1[k]) continue;
    const int32_t mk = B->m[k], nk = B->n[k];
    if (solve_lds_bytes_of(mk, nk) > LPX_BATCH_LDS_BYTES) return too_large_for_phase1("lpx_batch_solve", k, mk, nk);
    if (restore_order) {
      const int32_t* ok = restore_order + (int64_t)k * B->n_max;
      const int32_t len = restore_order_len ? restore_order_len[k] : -1;
      if (int rc = check_order("lpx_batch_solve", k, mk, nk, ok, len)) return rc;
      olen[k] = len < 0 ? nk : len;
      std::copy(ok, ok + olen[k], order.begin() + (int64_t)k * pitch);
    } else {
      olen[k] = nk;
      if (nk > 0) lpx_java_default_name_order(nk, order.data() + (int64_t)k * pitch);
    }
  }
  init_results(results, count);
  DeviceRestore keep_device;
  HIP_TRY(hipSetDevice(B->device));
  const size_t cnt = (size_t)count;
  if (maximize) HIP_TRY(hipMemcpyAsync(B->d_max.get(), maximize, cnt * sizeof(int32_t), hipMemcpyHostToDevice, B->stream));
  HIP_TRY(hipMemcpyAsync(B->d_order.get(), order.data(), order.size() * sizeof(int32_t), hipMemcpyHostToDevice, B->stream));
  HIP_TRY(hipMemcpyAsync(B->d_olen.get(), olen.data(), cnt * sizeof(int32_t), hipMemcpyHostToDevice, B->stream));
  const LaunchShape shape = batch_shape(B, true);
  lpxk::BatchSolveArgs a{};
  a.count = count;
  a.m = B->d_m.get();
  a.n = B->d_n.get();
  a.offset = B->d_offset.get();
  a.image = B->d_image.get();
  a.maximize = maximize ? B->d_max.get() : nullptr;
  a.phase1 = B->d_p1.get();
  a.order = B->d_order.get();
  a.order_len = B->d_olen.get();
  a.order_pitch = pitch;
  B->scalars.bind(a, count);
  a.max_pivots = max_pivots < 0 ? -1 : max_pivots;
  a.dantzig = B->pricing == 1;
  a.fused = B->fused;
  a.lds_bytes = (int32_t)shape.lds_bytes;
  a.threads = shape.threads;
  B->state = 2;
  const double t0 = now_s();   // behind uploads that may still be on their way: they count
  HIP_TRY(lpxk::launch_batch_solve(a, B->stream));
  HIP_TRY(hipStreamSynchronize(B->stream));
  const double t_pivots = now_s() - t0;
  if (int rc = B->scalars.fetch(B->stream)) return rc;
  bool device_error = false;
  for (int32_t k = 0; k < count; k++) {
    device_error |= B->scalars.decode(k, !maximize || maximize[k] != 0, results[k]);
    B->n_cur[k] = B->scalars.n_final(k);
  }
  stamp_seconds(results, count, t_start, t_pivots);
  if (device_error) return fail(LPX_DEVICE_ERROR, "lpx_batch_solve: the kernel and the host disagree about an LP's layout");
  return 0;
}

// x and perm of every LP from ONE copy of the images
extern "C" int lpx_batch_solutions(lpx_batch* B, double* x_out, int32_t* perm_out) {
  if (!B) return fail(LPX_BAD_ARGUMENT, "lpx_batch_solutions: NULL handle");
  if ((!x_out && !perm_out) || B->count == 0) return 0;
  DeviceRestore keep_device;
  std::vector<double> img;
  if (int rc = read_images(B, img)) return rc;
  for (int32_t k = 0; k < B->count; k++) write_solution(B, img, k, k, x_out, perm_out);
  return 0;
}

// What the launch of lpx_batch_simplex_loop / of lpx_batch_solve on this handle looks like (scripts/bench_batch.py): not
// part of include/lpx.h
extern "C" int lpxi_batch_launch_info(lpx_batch* B, int32_t* threads, int32_t* lds_bytes, int32_t* blocks_per_cu) {
  return launch_info("lpxi_batch_launch_info", B, false, threads, lds_bytes, blocks_per_cu);
}

extern "C" int lpxi_batch_solve_launch_info(lpx_batch* B, int32_t* threads, int32_t* lds_bytes, int32_t* blocks_per_cu) {
  return launch_info("lpxi_batch_solve_launch_info", B, true, threads, lds_bytes, blocks_per_cu);
}

// LPSolver.solve (LPSolver.java:78) for `count` standard forms.  The forms with min b >= 0 (no phase 1, :119) become one
// batch: c negated for `min` on a private copy (:86-89), slack form with the identity permutation (:248-272), ONE launch
// of the loop (:96-114).  The others take lpx_solve one by one (auxiliary LP, restoreInitialLP), into the same results.
extern "C" int lpx_solve_batch(int32_t count, int32_t m_max, int32_t n_max, const int32_t* m, const int32_t* n,
                               const double* A, int64_t lda, int64_t strideA, const double* b, const double* c,
                               const int32_t* maximize, const lpx_solve_options* opts, lpx_solve_result* results,
                               int32_t* n_in_batch) {
  if (n_in_batch) *n_in_batch = 0;
  const Forms F{count, m_max, n_max, m, n, A, lda, strideA, b, c, maximize};
  lpx_solve_options o;
  if (int rc = check_one_shot("lpx_solve_batch", F, true, results, "", opts, o)) return rc;
  const double t_start = now_s();
  init_results(results, count);
  std::vector<int32_t> in_batch, alone;
  for (int32_t k = 0; k < count; k++) (F.phase1(k) ? alone : in_batch).push_back(k);
  double t_pivots = 0.0;
  const int32_t nb = (int32_t)in_batch.size();
  if (nb > 0) {
    const Gathered G(F, in_batch, true);
    DeviceRestore keep_device;
    BatchGuard guard;
    if (int rc = G.create(o, guard)) return rc;
    const lpx_batch* B = guard.get();
    std::vector<int64_t> done(nb);
    std::vector<int32_t> st(nb);
    const double t0 = now_s();
    if (int rc = lpx_batch_simplex_loop(guard.get(), o.max_pivots < 0 ? -1 : o.max_pivots, done.data(), st.data(), nullptr)) return rc;
    t_pivots = now_s() - t0;
    std::vector<double> img;
    if (int rc = read_images(B, img)) return rc;
    for (int32_t t = 0; t < nb; t++) {   // the loop knows no phase 1: phase1_used, pivots_phase1 and x0_slot stay as initialised
      lpx_solve_result& r = results[in_batch[t]];
      fill_objective(r, img[(size_t)B->offset[t] + lpxk::batch_layout(G.m[t], G.n[t]).v], F.maximizes(in_batch[t]));
      r.pivots_phase2 = done[t];
      r.status = st[t];
    }
  }
  if (n_in_batch) *n_in_batch = nb;
  if (int rc = solve_alone(F, alone, o, results, nullptr, nullptr, t_pivots)) return rc;
  stamp_seconds(results, count, t_start, t_pivots);
  return 0;
}

// LPSolver.solve for `count` standard forms with phase 1 INSIDE the batch kernel: every form that fits k_batch_solve
// (lpx_batch_solve_lds_bytes where minInB finds a negative b, lpx_batch_lds_bytes otherwise) goes through one handle and
// one launch; a phase-1 form whose auxiliary LP does not fit takes lpx_solve, as in lpx_solve_batch.
extern "C" int lpx_solve_batch_all(int32_t count, int32_t m_max, int32_t n_max, const int32_t* m, const int32_t* n,
                                   const double* A, int64_t lda, int64_t strideA, const double* b, const double* c,
                                   const int32_t* maximize, const lpx_solve_options* opts, lpx_solve_result* results,
                                   double* x_out, int32_t* perm_out, int32_t* n_in_batch) {
  const char* who = "lpx_solve_batch_all";
  if (n_in_batch) *n_in_batch = 0;
  const Forms F{count, m_max, n_max, m, n, A, lda, strideA, b, c, maximize};
  lpx_solve_options o;
  if (int rc = check_one_shot(who, F, false, results, "opts->", opts, o)) return rc;
  std::vector<int32_t> in_batch, alone;
  for (int32_t k = 0; k < count; k++) {
    const int32_t mk = F.rows(k), nk = F.cols(k);
    const bool p1 = F.phase1(k);
    if (p1 && o.restore_order)
      if (int rc = check_order(who, k, mk, nk, o.restore_order, o.restore_order_len)) return rc;
    (p1 && solve_lds_bytes_of(mk, nk) > LPX_BATCH_LDS_BYTES ? alone : in_batch).push_back(k);
  }
  const double t_start = now_s();
  init_results(results, count);
  double t_pivots = 0.0;
  const int32_t nb = (int32_t)in_batch.size();
  if (nb > 0) {
    const Gathered G(F, in_batch, false);   // k_batch_solve negates c for `min` itself
    std::vector<int32_t> bmax(nb), border, blen;
    for (int32_t t = 0; t < nb; t++) bmax[t] = F.maximizes(in_batch[t]);
    if (o.restore_order) {   // the one order for every phase-1 form, as lpx_solve_batch hands it to lpx_solve
      border.assign((size_t)nb * n_max, 0);
      blen.assign(nb, 0);
      for (int32_t t = 0; t < nb; t++) {
        blen[t] = std::min(o.restore_order_len < 0 ? G.n[t] : o.restore_order_len, G.n[t]);
        std::copy(o.restore_order, o.restore_order + blen[t], border.begin() + (size_t)t * n_max);
      }
    }
    DeviceRestore keep_device;
    BatchGuard guard;
    if (int rc = G.create(o, guard)) return rc;
    lpx_batch* B = guard.get();
    std::vector<lpx_solve_result> res(nb);
    if (int rc = lpx_batch_solve(B, bmax.data(), o.max_pivots, o.restore_order ? border.data() : nullptr,
                                 o.restore_order ? blen.data() : nullptr, res.data()))
      return rc;
    t_pivots = res[0].seconds_pivots;
    std::vector<double> img;
    if (x_out || perm_out)
      if (int rc = read_images(B, img)) return rc;
    for (int32_t t = 0; t < nb; t++) {
      results[in_batch[t]] = res[t];
      if (x_out || perm_out) write_solution(B, img, t, in_batch[t], x_out, perm_out);   // as lpx_solve: only an m x n state
    }
  }
  if (n_in_batch) *n_in_batch = nb;
  if (int rc = solve_alone(F, alone, o, results, x_out, perm_out, t_pivots)) return rc;
  stamp_seconds(results, count, t_start, t_pivots);
  return 0;
}

// ---- scenario batches: ONE constraint matrix, many (b, c) -- k_batch_scenarios ---------------------------------------------
// The handle keeps the matrix on the device at pitch n.  A solve uploads b and c as they are (a strided copy, no host
// gather), a flag word per scenario and the one restore order; the kernel writes x, perm and seven scalars per scenario.
// The per-scenario buffers grow to the largest count seen.
struct lpx_scenarios {
  int device = 0;
  int32_t m = 0, n = 0;
  int fused = 0, pricing = 0;
  hipStream_t stream = nullptr;
  DeviceBuf<double> d_A;
  DeviceBuf<int32_t> d_order;
  int32_t cap = 0;   // scenarios the buffers below hold
  DeviceBuf<double> d_b, d_c, d_x;
  DeviceBuf<int32_t> d_flags, d_perm;
  SolveScalars scalars;
  // re-solve from a shared basis (lpx_scenarios_set_basis): the eta file of the crash, the matrix and the permutation at
  // the basis; per scenario the route k_batch_resolve took
  bool has_basis = false;
  int32_t n_eta = 0;
  DeviceBuf<double> d_eta, d_A_basis;
  DeviceBuf<int32_t> d_perm_basis, d_wanted, d_info, d_route;   // d_route: per scenario, sized with the buffers under `cap`

  // nothing is allocated before the stream exists; the members free themselves after this body
  ~lpx_scenarios() {
    if (!stream) return;
    (void)hipSetDevice(device);
    (void)hipStreamDestroy(stream);
  }
};

namespace {

using ScenariosGuard = std::unique_ptr<lpx_scenarios>;

// the shape and the matrix of a scenario batch
int check_scenario_matrix(const char* who, int32_t m, int32_t n, const double* A, int64_t lda, int device) {
  if (m < 0 || n < 0) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": negative dimension");
  if (lda < n) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": lda < n");
  if (m > 0 && n > 0 && !A) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": NULL array where data is due (A)");
  if (device < 0) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": negative device");
  const int64_t need = lds_bytes_of(m, n);
  if (need > LPX_BATCH_LDS_BYTES) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: the shape %d x %d needs %lld bytes of LDS, a workgroup has %d", who, m, n, (long long)need,
             LPX_BATCH_LDS_BYTES);
    return fail(LPX_BAD_ARGUMENT, msg);
  }
  return 0;
}

// A solve or a re-solve as the ABI passes it: `count` scenarios, b and c at their pitches (0: one vector), the budget,
// the restore order (NULL: the default) and where the answers go (x_out, perm_out: NULL for none); then what
// check_scenario_solve makes of it
struct ScenarioCall {
  int32_t count;
  const double *b, *c;
  int64_t ldb, ldc;
  int64_t max_pivots;
  const int32_t* restore_order;
  int32_t restore_order_len;
  lpx_solve_result* results;
  double* x_out;
  int32_t* perm_out;
  std::vector<int32_t> flags;   // [count] bit 0 = maximise, bit 1 = the scenario needs the auxiliary LP
  bool any_p1 = false;          // some scenario does
};

// the arguments of one solve on an m x n matrix; fills call.flags -- bit 1: minInB (LPSolver.java:375-386, the rule of
// Forms::phase1) finds a negative entry in the scenario's b -- and call.any_p1
int check_scenario_solve(const char* who, int32_t m, int32_t n, const int32_t* maximize, ScenarioCall& call) {
  const int32_t count = call.count;
  const double* b = call.b;
  const int64_t ldb = call.ldb;
  if (count < 0) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": negative count");
  if (ldb != 0 && ldb < m) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": ldb is neither 0 nor >= m");
  if (call.ldc != 0 && call.ldc < n) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": ldc is neither 0 nor >= n");
  if (count > 0 && !call.results) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": results is NULL");
  if (count > 0 && ((m > 0 && !b) || (n > 0 && !call.c)))
    return fail(LPX_BAD_ARGUMENT, std::string(who) + ": NULL array where data is due (b or c)");
  if (call.restore_order)
    if (int rc = check_order(who, 0, m, n, call.restore_order, call.restore_order_len)) return rc;
  call.flags.assign((size_t)std::max(count, 0), 0);
  call.any_p1 = false;
  const bool aux_fits = solve_lds_bytes_of(m, n) <= LPX_BATCH_LDS_BYTES;
  for (int32_t k = 0; k < count; k++) {
    const double* bk = b ? b + (int64_t)k * ldb : nullptr;
    const Forms one{1, m, n, nullptr, nullptr, nullptr, 0, 0, bk, nullptr, nullptr};
    const bool p1 = m > 0 && one.phase1(0);
    if (p1 && !aux_fits) {
      char msg[240];
      snprintf(msg, sizeof msg, "%s: scenario %d of shape %d x %d needs phase 1 and with it %lld bytes of LDS, a workgroup has %d",
               who, k, m, n, (long long)solve_lds_bytes_of(m, n), LPX_BATCH_LDS_BYTES);
      return fail(LPX_BAD_ARGUMENT, msg);
    }
    call.any_p1 |= p1;
    call.flags[k] = (!maximize || maximize[k] != 0 ? 1 : 0) | (p1 ? 2 : 0);
  }
  return 0;
}

// a failure leaves `out` empty and nothing allocated
int scenarios_create_checked(int32_t m, int32_t n, const double* A, int64_t lda, int device, ScenariosGuard& out) {
  ScenariosGuard guard(new lpx_scenarios());
  lpx_scenarios* S = guard.get();
  S->device = device;
  S->m = m;
  S->n = n;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreateWithFlags(&S->stream, hipStreamNonBlocking));
  HIP_TRY(S->d_A.alloc(std::max<size_t>((size_t)m * n, 1)));
  HIP_TRY(S->d_order.alloc((size_t)std::max(n, 1)));
  if (m > 0 && n > 0) {
    HIP_TRY(hipMemcpy2DAsync(S->d_A.get(), (size_t)n * sizeof(double), A, (size_t)lda * sizeof(double), (size_t)n * sizeof(double),
                             (size_t)m, hipMemcpyHostToDevice, S->stream));
    HIP_TRY(hipStreamSynchronize(S->stream));   // the caller's A is free again
  }
  out = std::move(guard);
  return 0;
}

// room for `count` scenarios: the per-scenario buffers grow to the largest count seen
int scenarios_reserve(lpx_scenarios* S, int32_t count) {
  if (count <= S->cap) return 0;
  S->cap = 0;   // until every buffer has its new size
  const size_t cnt = (size_t)count, m = (size_t)S->m, n = (size_t)S->n;
  HIP_TRY(S->d_b.alloc(std::max<size_t>(cnt * m, 1)));
  HIP_TRY(S->d_c.alloc(std::max<size_t>(cnt * n, 1)));
  HIP_TRY(S->d_x.alloc(std::max<size_t>(cnt * n, 1)));
  HIP_TRY(S->d_flags.alloc(cnt));
  HIP_TRY(S->d_perm.alloc(std::max<size_t>(cnt * (n + m), 1)));
  HIP_TRY(S->d_route.alloc(cnt));
  if (int rc = S->scalars.reserve(cnt)) return rc;
  S->cap = count;
  return 0;
}

// `rows` vectors of `len` doubles at the host pitch ld (0: one vector) to the device at pitch len (0 stays 0)
int upload_vectors(lpx_scenarios* S, double* dst, const double* src, int64_t ld, int32_t len, int32_t rows) {
  if (len == 0 || rows == 0) return 0;
  const size_t w = (size_t)len * sizeof(double);
  if (ld == 0) HIP_TRY(hipMemcpyAsync(dst, src, w, hipMemcpyHostToDevice, S->stream));
  else if (ld == len) HIP_TRY(hipMemcpyAsync(dst, src, w * (size_t)rows, hipMemcpyHostToDevice, S->stream));
  else HIP_TRY(hipMemcpy2DAsync(dst, w, src, (size_t)ld * sizeof(double), w, (size_t)rows, hipMemcpyHostToDevice, S->stream));
  return 0;
}

// What lpx_scenarios_solve and lpx_scenarios_resolve do alike, up to the end of their launch.  Room for the call's
// scenarios; b, c and the flags go up, and the a.order_len entries of `order` where the kernel reads a restore order.
// The fields of `a` that every scenario kernel reads are set here; A and what only one kernel reads are the caller's.
// Then `launch` alone between two synchronises: t_pivots is the seconds of that window.
template <class Args, class Launch>
int launch_scenarios(lpx_scenarios* S, const ScenarioCall& call, Args& a, LaunchShape shape, const int32_t* order, Launch launch,
                     double& t_pivots) {
  const int32_t m = S->m, n = S->n, count = call.count;
  HIP_TRY(hipSetDevice(S->device));
  if (int rc = scenarios_reserve(S, count)) return rc;
  if (int rc = upload_vectors(S, S->d_b.get(), call.b, call.ldb, m, count)) return rc;
  if (int rc = upload_vectors(S, S->d_c.get(), call.c, call.ldc, n, count)) return rc;
  HIP_TRY(hipMemcpyAsync(S->d_flags.get(), call.flags.data(), (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, S->stream));
  if (a.order_len > 0)
    HIP_TRY(hipMemcpyAsync(S->d_order.get(), order, (size_t)a.order_len * sizeof(int32_t), hipMemcpyHostToDevice, S->stream));
  a.count = count;
  a.m = m;
  a.n = n;
  a.b = S->d_b.get();
  a.c = S->d_c.get();
  a.ldb = call.ldb == 0 ? 0 : m;
  a.ldc = call.ldc == 0 ? 0 : n;
  a.flags = S->d_flags.get();
  S->scalars.bind(a, count);
  a.x_out = call.x_out ? S->d_x.get() : nullptr;
  a.perm_out = call.perm_out ? S->d_perm.get() : nullptr;
  a.max_pivots = call.max_pivots < 0 ? -1 : call.max_pivots;
  a.dantzig = S->pricing == 1;
  a.fused = S->fused;
  a.lds_bytes = (int32_t)shape.lds_bytes;
  a.threads = shape.threads;
  HIP_TRY(hipStreamSynchronize(S->stream));   // the uploads are through: seconds_pivots is the launch alone
  const double t0 = now_s();
  HIP_TRY(launch());
  HIP_TRY(hipStreamSynchronize(S->stream));
  t_pivots = now_s() - t0;
  return 0;
}

// row t of xs (pitch xw) and of ps (pitch pw) into row k of x_out and perm_out; a NULL source is not wanted
void copy_row(size_t xw, size_t pw, const double* xs, const int32_t* ps, size_t t, double* x_out, int32_t* perm_out, size_t k) {
  if (xs && xw > 0) memcpy(x_out + k * xw, xs + t * xw, xw * sizeof(double));
  if (ps && pw > 0) memcpy(perm_out + k * pw, ps + t * pw, pw * sizeof(int32_t));
}

// x and perm of the scenarios k with keep(k), from the rows the kernel wrote on the device, into the caller's x_out and
// perm_out (either may be NULL).  All of them (the usual case): one copy each straight into the caller's arrays; else
// through a host copy, row by row, and the rows of the others stay as they are
template <class Keep>
int download_rows(lpx_scenarios* S, int32_t count, Keep keep, double* x_out, int32_t* perm_out) {
  const size_t cnt = (size_t)count, xw = (size_t)S->n, pw = (size_t)S->n + S->m;
  bool all = true;
  for (int32_t k = 0; k < count; k++) all &= keep(k);
  std::vector<double> hx(!all && x_out ? cnt * xw : 0);
  std::vector<int32_t> hp(!all && perm_out ? cnt * pw : 0);
  if (x_out && xw > 0)
    HIP_TRY(hipMemcpyAsync(all ? x_out : hx.data(), S->d_x.get(), cnt * xw * sizeof(double), hipMemcpyDeviceToHost, S->stream));
  if (perm_out && pw > 0)
    HIP_TRY(hipMemcpyAsync(all ? perm_out : hp.data(), S->d_perm.get(), cnt * pw * sizeof(int32_t), hipMemcpyDeviceToHost, S->stream));
  HIP_TRY(hipStreamSynchronize(S->stream));
  for (int32_t k = 0; !all && k < count; k++)
    if (keep(k)) copy_row(xw, pw, x_out ? hx.data() : nullptr, perm_out ? hp.data() : nullptr, k, x_out, perm_out, k);
  return 0;
}

// the checked core of lpx_scenarios_solve: count > 0
int scenarios_solve_checked(const char* who, lpx_scenarios* S, const ScenarioCall& call) {
  const double t_start = now_s();
  const int32_t m = S->m, n = S->n, count = call.count;
  std::vector<int32_t> order((size_t)std::max(n, 1), 0);
  lpxk::BatchScenarioArgs a{};
  a.A = S->d_A.get();
  a.order = S->d_order.get();
  a.order_len = n;
  if (call.restore_order) {
    a.order_len = call.restore_order_len < 0 ? n : call.restore_order_len;
    std::copy(call.restore_order, call.restore_order + a.order_len, order.begin());
  } else if (n > 0) {
    lpx_java_default_name_order(n, order.data());
  }
  init_results(call.results, count);
  double t_pivots = 0.0;
  auto launch = [&] { return lpxk::launch_batch_scenarios(a, S->stream); };
  if (int rc = launch_scenarios(S, call, a, scenario_shape(m, n, call.any_p1), order.data(), launch, t_pivots)) return rc;
  if (int rc = S->scalars.fetch(S->stream)) return rc;
  bool device_error = false;
  for (int32_t k = 0; k < count; k++) device_error |= S->scalars.decode(k, (call.flags[k] & 1) != 0, call.results[k]);
  if (device_error) {
    stamp_seconds(call.results, count, t_start, t_pivots);
    return fail(LPX_DEVICE_ERROR, std::string(who) + ": the kernel and the host disagree about a scenario's layout");
  }
  // the kernel wrote the rows of the scenarios that ended m x n and no others
  auto ended_mxn = [&](int32_t k) { return S->scalars.n_final(k) == n; };
  if (int rc = download_rows(S, count, ended_mxn, call.x_out, call.perm_out)) return rc;
  stamp_seconds(call.results, count, t_start, t_pivots);
  return 0;
}

// ---- re-solve from a shared basis -----------------------------------------------------------------------------------------
// m variable ids, each in [0, n + m), all distinct
int check_basis(const char* who, int32_t m, int32_t n, const int32_t* basis) {
  std::vector<char> seen((size_t)n + m, 0);
  char msg[200];
  for (int32_t i = 0; i < m; i++) {
    const int32_t id = basis[i];
    if (id < 0 || id >= n + m) {
      snprintf(msg, sizeof msg, "%s: basis entry %d names variable id %d outside 0..%d", who, i, id, n + m - 1);
      return fail(LPX_BAD_ARGUMENT, msg);
    }
    if (seen[id]) {
      snprintf(msg, sizeof msg, "%s: basis entry %d repeats variable id %d", who, i, id);
      return fail(LPX_BAD_ARGUMENT, msg);
    }
    seen[id] = 1;
  }
  return 0;
}

// the checked core of lpx_scenarios_set_basis: ONE workgroup of k_scenarios_crash brings the handle's matrix to the basis
int scenarios_set_basis_checked(const char* who, lpx_scenarios* S, const int32_t* basis, int32_t* crash_pivots_out) {
  S->has_basis = false;
  S->n_eta = 0;
  if (crash_pivots_out) *crash_pivots_out = 0;
  if (!basis) return 0;
  const int32_t m = S->m, n = S->n;
  std::vector<int32_t> wanted((size_t)std::max(n + m, 1), 0);
  for (int32_t i = 0; i < m; i++) wanted[basis[i]] = 1;
  HIP_TRY(hipSetDevice(S->device));
  if (!S->d_eta.get()) {
    const size_t etas = (size_t)std::min(m, n) * (size_t)lpxk::eta_stride(m, n);
    HIP_TRY(S->d_eta.alloc(std::max<size_t>(etas, 1)));
    HIP_TRY(S->d_A_basis.alloc(std::max<size_t>((size_t)m * n, 1)));
    HIP_TRY(S->d_perm_basis.alloc(wanted.size()));
    HIP_TRY(S->d_wanted.alloc(wanted.size()));
    HIP_TRY(S->d_info.alloc(2));
  }
  HIP_TRY(hipMemcpyAsync(S->d_wanted.get(), wanted.data(), wanted.size() * sizeof(int32_t), hipMemcpyHostToDevice, S->stream));
  const LaunchShape shape = scenario_shape(m, n, false);
  lpxk::ScenarioCrashArgs a{};
  a.count = 1;
  a.m = m;
  a.n = n;
  a.A = S->d_A.get();
  a.wanted = S->d_wanted.get();
  a.A_out = S->d_A_basis.get();
  a.perm_out = S->d_perm_basis.get();
  a.eta = S->d_eta.get();
  a.info = S->d_info.get();
  a.fused = S->fused;
  a.lds_bytes = (int32_t)shape.lds_bytes;
  a.threads = shape.threads;
  HIP_TRY(lpxk::launch_scenarios_crash(a, S->stream));
  int32_t info[2] = {0, -2};
  HIP_TRY(hipMemcpyAsync(info, S->d_info.get(), sizeof info, hipMemcpyDeviceToHost, S->stream));
  HIP_TRY(hipStreamSynchronize(S->stream));
  if (info[1] == -2) return fail(LPX_DEVICE_ERROR, std::string(who) + ": the kernel and the host disagree about the layout");
  if (info[1] >= 0) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: basis is singular at variable id %d", who, info[1]);
    return fail(LPX_BAD_ARGUMENT, msg);
  }
  S->n_eta = info[0];
  S->has_basis = true;
  if (crash_pivots_out) *crash_pivots_out = info[0];
  return 0;
}

// The scenarios k_batch_resolve routed cold (none: nothing to do): lpx_scenarios_solve on their rows of b and c,
// gathered; results, x and perm scattered back, and the seconds of that launch added to t_pivots
int resolve_cold(const char* who, lpx_scenarios* S, const ScenarioCall& call, const std::vector<int32_t>& route, double& t_pivots) {
  const int32_t m = S->m, n = S->n;
  const int64_t ldb = call.ldb, ldc = call.ldc;
  const size_t xw = (size_t)n, pw = (size_t)n + m;
  std::vector<int32_t> cold;
  for (int32_t k = 0; k < call.count; k++)
    if (route[k] == LPX_ROUTE_COLD) cold.push_back(k);
  if (cold.empty()) return 0;
  const int32_t nc = (int32_t)cold.size();
  std::vector<double> gb(ldb == 0 ? 0 : (size_t)nc * m), gc(ldc == 0 ? 0 : (size_t)nc * n);
  std::vector<lpx_solve_result> res(nc);
  std::vector<double> tx(call.x_out ? (size_t)nc * xw : 0);
  std::vector<int32_t> tp((size_t)nc * pw, -1);   // a row the solve leaves alone (ended inside phase 1) still starts with -1
  ScenarioCall gathered{nc, ldb == 0 ? call.b : gb.data(), ldc == 0 ? call.c : gc.data(), ldb == 0 ? 0 : m, ldc == 0 ? 0 : n,
                        call.max_pivots, call.restore_order, call.restore_order_len, res.data(),
                        tx.empty() ? nullptr : tx.data(), tp.empty() ? nullptr : tp.data()};
  for (int32_t t = 0; t < nc; t++) {
    const int32_t k = cold[t];
    if (ldb != 0 && m > 0) memcpy(&gb[(size_t)t * m], call.b + k * ldb, (size_t)m * sizeof(double));
    if (ldc != 0 && n > 0) memcpy(&gc[(size_t)t * n], call.c + k * ldc, (size_t)n * sizeof(double));
    gathered.flags.push_back(call.flags[k]);
    gathered.any_p1 |= (call.flags[k] & 2) != 0;
  }
  if (int rc = scenarios_solve_checked(who, S, gathered)) return rc;
  t_pivots += res[0].seconds_pivots;
  for (int32_t t = 0; t < nc; t++) {
    call.results[cold[t]] = res[t];
    if (pw > 0 && tp[(size_t)t * pw] < 0) continue;
    copy_row(xw, pw, tx.empty() ? nullptr : tx.data(), call.perm_out ? tp.data() : nullptr, t, call.x_out, call.perm_out, cold[t]);
  }
  return 0;
}

// the checked core of lpx_scenarios_resolve: the handle has a basis
int scenarios_resolve_checked(const char* who, lpx_scenarios* S, const ScenarioCall& call, int32_t* route_out) {
  const double t_start = now_s();
  const int32_t m = S->m, n = S->n, count = call.count;
  lpx_solve_result* results = call.results;
  init_results(results, count);
  lpxk::BatchResolveArgs a{};
  a.A = S->d_A_basis.get();
  a.perm0 = S->d_perm_basis.get();
  a.eta = S->d_eta.get();
  a.n_eta = S->n_eta;
  double t_pivots = 0.0;
  auto launch = [&] {
    a.route = S->d_route.get();   // one of the per-scenario buffers: there for this count only now
    return lpxk::launch_batch_resolve(a, S->stream);
  };
  if (int rc = launch_scenarios(S, call, a, scenario_shape(m, n, false), nullptr, launch, t_pivots)) return rc;
  std::vector<int32_t> route(count);
  HIP_TRY(hipMemcpyAsync(route.data(), S->d_route.get(), route.size() * sizeof(int32_t), hipMemcpyDeviceToHost, S->stream));
  if (int rc = S->scalars.fetch(S->stream)) return rc;
  // a warm scenario's phase1_used and x0_slot are decoded like the rest: k_batch_resolve writes 0 and -1 there
  auto warm = [&](int32_t k) { return route[k] != LPX_ROUTE_COLD; };
  bool device_error = false;
  for (int32_t k = 0; k < count; k++)
    if (warm(k)) device_error |= S->scalars.decode(k, (call.flags[k] & 1) != 0, results[k]);
  if (device_error) {
    stamp_seconds(results, count, t_start, t_pivots);
    return fail(LPX_DEVICE_ERROR, std::string(who) + ": the kernel and the host disagree about a scenario's layout");
  }
  // x and perm of the warm scenarios: their final state is always m x n.  The cold solve reuses the device rows
  if (int rc = download_rows(S, count, warm, call.x_out, call.perm_out)) return rc;
  if (int rc = resolve_cold(who, S, call, route, t_pivots)) return rc;
  if (route_out) memcpy(route_out, route.data(), route.size() * sizeof(int32_t));
  stamp_seconds(results, count, t_start, t_pivots);
  return 0;
}

// create, `work` on the handle, destroy: the one-shot scenario calls behind their checks.  The times are those of the
// whole call, creation included
template <class Work>
int with_scenarios(int32_t m, int32_t n, const double* A, int64_t lda, const lpx_solve_options& o, const ScenarioCall& call,
                   Work work) {
  const double t_start = now_s();
  DeviceRestore keep_device;
  ScenariosGuard S;
  if (int rc = scenarios_create_checked(m, n, A, lda, o.device, S)) return rc;
  S->fused = o.fused > 0;   // 0 = the library's choice by size = two roundings here, as in lpx_solve at these sizes
  S->pricing = o.pricing;
  if (int rc = work(S.get())) return rc;
  stamp_seconds(call.results, call.count, t_start, call.results[0].seconds_pivots);
  return 0;
}

// the launch-info call of a scenario kernel on this handle
template <class Occupancy>
int scenarios_launch_info(const char* who, lpx_scenarios* S, bool phase1, Occupancy occupancy, int32_t* threads,
                          int32_t* lds_bytes, int32_t* blocks_per_cu) {
  if (!S) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": NULL handle");
  return report_launch(S->device, scenario_shape(S->m, S->n, phase1), occupancy, threads, lds_bytes, blocks_per_cu);
}

}  // namespace

extern "C" int lpx_scenarios_create(int32_t m, int32_t n, const double* A, int64_t lda, int device, lpx_scenarios** out) {
  if (!out) return fail(LPX_BAD_ARGUMENT, "lpx_scenarios_create: out is NULL");
  *out = nullptr;
  if (int rc = check_scenario_matrix("lpx_scenarios_create", m, n, A, lda, device)) return rc;
  DeviceRestore keep_device;
  ScenariosGuard S;
  const int rc = scenarios_create_checked(m, n, A, lda, device, S);
  *out = S.release();
  return rc;
}

extern "C" void lpx_scenarios_destroy(lpx_scenarios* S) {
  DeviceRestore keep_device;
  delete S;
}

extern "C" int lpx_scenarios_set_option(lpx_scenarios* S, int32_t key, int64_t value) {
  if (!S) return fail(LPX_BAD_ARGUMENT, "lpx_scenarios_set_option: NULL handle");
  if (key != LPX_OPT_FUSED || value < 0 || value > 2)
    return fail(LPX_BAD_ARGUMENT, "lpx_scenarios_set_option: only LPX_OPT_FUSED (0, 1, 2) applies to a scenario batch");
  if (S->fused != (value == 1)) S->has_basis = false;   // the matrix at the basis carries the roundings of the mode it was made in
  S->fused = value == 1;   // 2 = by size: a shape that fits a workgroup is far below the switch, i.e. 0
  return 0;
}

extern "C" int lpx_scenarios_set_pricing(lpx_scenarios* S, int32_t pricing) {
  if (!S || (pricing != 0 && pricing != 1)) return fail(LPX_BAD_ARGUMENT, "lpx_scenarios_set_pricing: bad argument");
  S->pricing = pricing;
  return 0;
}

// LPSolver.solve (LPSolver.java:78) for `count` scenarios (b, c, max | min) of the handle's matrix in ONE launch of
// k_batch_scenarios; the handle is as it was afterwards
extern "C" int lpx_scenarios_solve(lpx_scenarios* S, int32_t count, const double* b, int64_t ldb, const double* c, int64_t ldc,
                                   const int32_t* maximize, int64_t max_pivots, const int32_t* restore_order,
                                   int32_t restore_order_len, lpx_solve_result* results, double* x_out, int32_t* perm_out) {
  const char* who = "lpx_scenarios_solve";
  if (!S) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": NULL handle");
  ScenarioCall call{count, b, c, ldb, ldc, max_pivots, restore_order, restore_order_len, results, x_out, perm_out};
  if (int rc = check_scenario_solve(who, S->m, S->n, maximize, call)) return rc;
  if (count == 0) return 0;
  DeviceRestore keep_device;
  return scenarios_solve_checked(who, S, call);
}

// create, solve, destroy
extern "C" int lpx_solve_scenarios(int32_t m, int32_t n, const double* A, int64_t lda, int32_t count, const double* b,
                                   int64_t ldb, const double* c, int64_t ldc, const int32_t* maximize,
                                   const lpx_solve_options* opts, lpx_solve_result* results, double* x_out, int32_t* perm_out) {
  const char* who = "lpx_solve_scenarios";
  lpx_solve_options o;
  if (int rc = take_options(who, "opts->", false, opts, o)) return rc;
  if (int rc = check_scenario_matrix(who, m, n, A, lda, o.device)) return rc;
  ScenarioCall call{count, b, c, ldb, ldc, o.max_pivots, o.restore_order, o.restore_order_len, results, x_out, perm_out};
  if (int rc = check_scenario_solve(who, m, n, maximize, call)) return rc;
  if (count == 0) return 0;
  return with_scenarios(m, n, A, lda, o, call, [&](lpx_scenarios* S) { return scenarios_solve_checked(who, S, call); });
}

// The basis every later lpx_scenarios_resolve starts from: m variable ids (perm's numbering), NULL clears it
extern "C" int lpx_scenarios_set_basis(lpx_scenarios* S, const int32_t* basis, int32_t* crash_pivots_out) {
  const char* who = "lpx_scenarios_set_basis";
  if (crash_pivots_out) *crash_pivots_out = 0;
  if (!S) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": NULL handle");
  if (basis)
    if (int rc = check_basis(who, S->m, S->n, basis)) return rc;
  DeviceRestore keep_device;
  return scenarios_set_basis_checked(who, S, basis, crash_pivots_out);
}

// lpx_scenarios_solve from the handle's basis: ONE launch of k_batch_resolve, then the scenarios it routed cold through
// the launch lpx_scenarios_solve makes
extern "C" int lpx_scenarios_resolve(lpx_scenarios* S, int32_t count, const double* b, int64_t ldb, const double* c, int64_t ldc,
                                     const int32_t* maximize, int64_t max_pivots, const int32_t* restore_order,
                                     int32_t restore_order_len, lpx_solve_result* results, double* x_out, int32_t* perm_out,
                                     int32_t* route_out) {
  const char* who = "lpx_scenarios_resolve";
  if (!S) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": NULL handle");
  ScenarioCall call{count, b, c, ldb, ldc, max_pivots, restore_order, restore_order_len, results, x_out, perm_out};
  if (int rc = check_scenario_solve(who, S->m, S->n, maximize, call)) return rc;
  if (!S->has_basis) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": the handle has no basis (lpx_scenarios_set_basis)");
  if (count == 0) return 0;
  DeviceRestore keep_device;
  return scenarios_resolve_checked(who, S, call, route_out);
}

// create, set_basis, resolve, destroy
extern "C" int lpx_solve_scenarios_from_basis(int32_t m, int32_t n, const double* A, int64_t lda, const int32_t* basis,
                                              int32_t count, const double* b, int64_t ldb, const double* c, int64_t ldc,
                                              const int32_t* maximize, const lpx_solve_options* opts, lpx_solve_result* results,
                                              double* x_out, int32_t* perm_out, int32_t* route_out) {
  const char* who = "lpx_solve_scenarios_from_basis";
  lpx_solve_options o;
  if (int rc = take_options(who, "opts->", false, opts, o)) return rc;
  if (int rc = check_scenario_matrix(who, m, n, A, lda, o.device)) return rc;
  if (!basis) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": basis is NULL");
  if (int rc = check_basis(who, m, n, basis)) return rc;
  ScenarioCall call{count, b, c, ldb, ldc, o.max_pivots, o.restore_order, o.restore_order_len, results, x_out, perm_out};
  if (int rc = check_scenario_solve(who, m, n, maximize, call)) return rc;
  if (count == 0) return 0;
  return with_scenarios(m, n, A, lda, o, call, [&](lpx_scenarios* S) {   // the crash counts into the times too
    if (int rc = scenarios_set_basis_checked(who, S, basis, nullptr)) return rc;
    return scenarios_resolve_checked(who, S, call, route_out);
  });
}

// What the launch of lpx_scenarios_resolve looks like for this handle, and the entries of its eta file
// (scripts/bench_scenarios_resolve.py): not part of include/lpx.h
extern "C" int lpxi_scenarios_resolve_launch_info(lpx_scenarios* S, int32_t* threads, int32_t* lds_bytes, int32_t* blocks_per_cu,
                                                  int32_t* etas) {
  if (int rc = scenarios_launch_info("lpxi_scenarios_resolve_launch_info", S, false, lpxk::batch_resolve_blocks_per_cu, threads,
                                     lds_bytes, blocks_per_cu))
    return rc;
  if (etas) *etas = S->has_basis ? S->n_eta : -1;
  return 0;
}

// What the launch of lpx_scenarios_solve looks like for this handle (scripts/bench_scenarios.py): not part of include/lpx.h
extern "C" int lpxi_scenarios_launch_info(lpx_scenarios* S, int32_t phase1, int32_t* threads, int32_t* lds_bytes,
                                          int32_t* blocks_per_cu) {
  return scenarios_launch_info("lpxi_scenarios_launch_info", S, phase1 != 0, lpxk::batch_scenarios_blocks_per_cu, threads,
                               lds_bytes, blocks_per_cu);
}
