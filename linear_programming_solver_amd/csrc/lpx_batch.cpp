// Batched solve behind the C ABI (include/lpx.h): many small LPs in ONE launch, one workgroup per LP with the LP's whole
// state in LDS (lpx_batch.inc: k_batch_simplex runs the loop, k_batch_solve the whole of LPSolver.solve with phase 1,
// k_batch_scenarios the same for many (b, c) on one matrix, k_scenarios_crash and k_batch_resolve the re-solve of such
// scenarios from a shared basis: lpx_scenarios at the end of this file).
// The handle keeps one HBM image per LP (lpxk::BatchLayout).  lpx_solve_batch and lpx_solve_batch_all are built from one
// set of pieces (Forms, check_one_shot, Gathered, solve_alone, stamp_seconds).  Every argument is checked before the first
// device call, so a bad call answers LPX_BAD_ARGUMENT on a machine without a GPU too.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lpx_internal.h"

namespace lpx_internal {
void round6_text(double v, char* out, size_t cap);   // lpx_solver.cpp
}

struct lpx_batch {
  int device = 0;
  int32_t count = 0, m_max = 0, n_max = 0;
  std::vector<int32_t> m, n;
  std::vector<int64_t> offset;      // first double of LP k's image; offset[count] = doubles of all images
  int32_t lds_bytes = 0;            // dynamic LDS of the launch: the largest LP's
  int32_t threads = 64;             // workgroup size chosen for the batch
  int fused = 0, pricing = 0;
  hipStream_t stream = nullptr;
  double* d_image = nullptr;
  int64_t *d_offset = nullptr, *d_pivots = nullptr;
  int32_t *d_m = nullptr, *d_n = nullptr, *d_status = nullptr, *d_track = nullptr;
  // lpx_batch_solve
  std::vector<int32_t> n_cur;       // columns of LP k now: n[k], or n[k] + 1 after a solve that ended inside phase 1
  std::vector<int32_t> need_p1;     // minInB of the b given at creation finds a negative entry: the image has room for n + 1 columns
  bool custom_start = false;        // created with a nonzero v or with perm: not the start of LPSolver.solve
  int state = 0;                    // 0: as created, 1: a loop has run, 2: solved
  int32_t solve_threads = 64;       // workgroup size of k_batch_solve: by the auxiliary shape where phase 1 is due
  // inputs and outputs of k_batch_solve, allocated with the handle: flags, orders, 4 int32 / 2 int64 / 1 double per LP
  int32_t *d_max = nullptr, *d_p1 = nullptr, *d_order = nullptr, *d_olen = nullptr, *d_si32 = nullptr;
  int64_t* d_si64 = nullptr;
  double* d_sv = nullptr;
};

namespace {

double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

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

void free_batch(lpx_batch* B) {
  if (!B) return;
  if (B->stream || B->d_image || B->d_offset) {
    (void)hipSetDevice(B->device);
    (void)hipFree(B->d_image);
    (void)hipFree(B->d_offset);
    (void)hipFree(B->d_pivots);
    (void)hipFree(B->d_m);
    (void)hipFree(B->d_n);
    (void)hipFree(B->d_status);
    (void)hipFree(B->d_track);
    (void)hipFree(B->d_max);
    (void)hipFree(B->d_p1);
    (void)hipFree(B->d_order);
    (void)hipFree(B->d_olen);
    (void)hipFree(B->d_si32);
    (void)hipFree(B->d_si64);
    (void)hipFree(B->d_sv);
    if (B->stream) (void)hipStreamDestroy(B->stream);
  }
  delete B;
}

struct BatchGuard {
  lpx_batch* B = nullptr;
  ~BatchGuard() { free_batch(B); }
};

// the checked core of lpx_batch_create (no argument checks: the callers have made them)
int create_checked(const Forms& F, const double* v, const int32_t* perm, int device, lpx_batch** out) {
  const int32_t count = F.count, m_max = F.m_max, n_max = F.n_max;
  BatchGuard guard;
  lpx_batch* B = guard.B = new lpx_batch();
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
  HIP_TRY(hipMalloc((void**)&B->d_image, std::max<size_t>((size_t)total, 2) * sizeof(double)));
  HIP_TRY(hipMalloc((void**)&B->d_offset, cnt * sizeof(int64_t)));
  HIP_TRY(hipMalloc((void**)&B->d_pivots, cnt * sizeof(int64_t)));
  HIP_TRY(hipMalloc((void**)&B->d_m, cnt * sizeof(int32_t)));
  HIP_TRY(hipMalloc((void**)&B->d_n, cnt * sizeof(int32_t)));
  HIP_TRY(hipMalloc((void**)&B->d_status, cnt * sizeof(int32_t)));
  HIP_TRY(hipMalloc((void**)&B->d_track, cnt * sizeof(int32_t)));
  HIP_TRY(hipMalloc((void**)&B->d_max, cnt * sizeof(int32_t)));
  HIP_TRY(hipMalloc((void**)&B->d_p1, cnt * sizeof(int32_t)));
  HIP_TRY(hipMalloc((void**)&B->d_order, cnt * (size_t)std::max(n_max, 1) * sizeof(int32_t)));
  HIP_TRY(hipMalloc((void**)&B->d_olen, cnt * sizeof(int32_t)));
  HIP_TRY(hipMalloc((void**)&B->d_si32, 4 * cnt * sizeof(int32_t)));
  HIP_TRY(hipMalloc((void**)&B->d_si64, 2 * cnt * sizeof(int64_t)));
  HIP_TRY(hipMalloc((void**)&B->d_sv, cnt * sizeof(double)));
  if (total > 0) HIP_TRY(hipMemcpyAsync(B->d_image, img.data(), (size_t)total * sizeof(double), hipMemcpyHostToDevice, B->stream));
  if (count > 0) {
    HIP_TRY(hipMemcpyAsync(B->d_offset, B->offset.data(), (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice, B->stream));
    HIP_TRY(hipMemcpyAsync(B->d_m, B->m.data(), (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, B->stream));
    HIP_TRY(hipMemcpyAsync(B->d_n, B->n.data(), (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, B->stream));
    HIP_TRY(hipMemcpyAsync(B->d_p1, B->need_p1.data(), (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, B->stream));
  }
  HIP_TRY(hipStreamSynchronize(B->stream));   // img goes out of scope
  guard.B = nullptr;
  *out = B;
  return 0;
}

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

void fill_objective(lpx_solve_result& r, double v, bool maximize) {
  if (!maximize) v = -v;                                                            // LPSolver.java:90
  r.objective = v;
  lpx_internal::round6_text(v, r.objective_text, sizeof r.objective_text);         // :113
  r.objective_rounded = strtod(r.objective_text, nullptr);
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
  HIP_TRY(hipMemcpyAsync(img.data(), B->d_image, img.size() * sizeof(double), hipMemcpyDeviceToHost, B->stream));
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
  DeviceRestore keep_device;
  HIP_TRY(hipSetDevice(B->device));
  const int t = threads_in_effect(B, solve);
  const int lds = solve ? (int)std::min<int64_t>(solve_launch_lds(B), INT32_MAX) : B->lds_bytes;
  if (threads) *threads = t;
  if (lds_bytes) *lds_bytes = lds;
  if (blocks_per_cu) *blocks_per_cu = solve ? lpxk::batch_solve_blocks_per_cu(t, lds) : lpxk::batch_blocks_per_cu(t, lds);
  return 0;
}

// The argument checks of a one-shot call in their order: shapes, arrays, results (and the flags where maximize_due), then
// the options into `o` (NULL: the defaults) without what a batch cannot honour; `field` is how `who` names those.
int check_one_shot(const char* who, const Forms& F, bool maximize_due, const lpx_solve_result* results, const char* field,
                   const lpx_solve_options* opts, lpx_solve_options& o) {
  if (int rc = check_forms(who, F)) return rc;
  if (F.count > 0 && (!results || (maximize_due && !F.maximize)))
    return fail(LPX_BAD_ARGUMENT, std::string(who) + (maximize_due ? ": results or maximize is NULL" : ": results is NULL"));
  o = lpx_solve_options{};
  o.max_pivots = -1;
  if (opts) o = *opts;
  const std::string f(field);
  if (o.keep_state || o.perm_out || o.x_out)
    return fail(LPX_BAD_ARGUMENT, std::string(who) + ": " + f + "keep_state, " + f + "perm_out and " + f + "x_out must be NULL");
  if (o.device < 0 || (o.pricing != 0 && o.pricing != 1)) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": bad device or pricing");
  return 0;
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
    if (int rc = create_checked(G, nullptr, nullptr, o.device, &guard.B)) return rc;
    guard.B->fused = o.fused > 0;   // 0 = the library's choice by size = two roundings here, as in lpx_solve at these sizes
    guard.B->pricing = o.pricing;
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
  return create_checked(F, v, perm, device, out);
}

extern "C" void lpx_batch_destroy(lpx_batch* B) {
  DeviceRestore keep_device;
  free_batch(B);
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
  if (track_slot) HIP_TRY(hipMemcpyAsync(B->d_track, track_slot, cnt * sizeof(int32_t), hipMemcpyHostToDevice, B->stream));
  else HIP_TRY(hipMemsetAsync(B->d_track, 0xff, cnt * sizeof(int32_t), B->stream));   // -1: nothing tracked
  lpxk::BatchArgs a{};
  a.count = B->count;
  a.m = B->d_m;
  a.n = B->d_n;
  a.offset = B->d_offset;
  a.image = B->d_image;
  a.pivots = B->d_pivots;
  a.status = B->d_status;
  a.track = B->d_track;
  a.max_pivots = max_pivots;
  a.dantzig = B->pricing == 1;
  a.fused = B->fused;
  a.lds_bytes = B->lds_bytes;
  a.threads = threads_in_effect(B);
  HIP_TRY(lpxk::launch_batch_simplex(a, B->stream));
  HIP_TRY(hipMemcpyAsync(pivots_done, B->d_pivots, cnt * sizeof(int64_t), hipMemcpyDeviceToHost, B->stream));
  HIP_TRY(hipMemcpyAsync(status, B->d_status, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, B->stream));
  if (track_slot) HIP_TRY(hipMemcpyAsync(track_slot, B->d_track, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, B->stream));
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
  HIP_TRY(hipMemcpyAsync(img.data(), B->d_image + B->offset[index], img.size() * sizeof(double), hipMemcpyDeviceToHost, B->stream));
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
  if (maximize) HIP_TRY(hipMemcpyAsync(B->d_max, maximize, cnt * sizeof(int32_t), hipMemcpyHostToDevice, B->stream));
  HIP_TRY(hipMemcpyAsync(B->d_order, order.data(), order.size() * sizeof(int32_t), hipMemcpyHostToDevice, B->stream));
  HIP_TRY(hipMemcpyAsync(B->d_olen, olen.data(), cnt * sizeof(int32_t), hipMemcpyHostToDevice, B->stream));
  lpxk::BatchSolveArgs a{};
  a.count = count;
  a.m = B->d_m;
  a.n = B->d_n;
  a.offset = B->d_offset;
  a.image = B->d_image;
  a.maximize = maximize ? B->d_max : nullptr;
  a.phase1 = B->d_p1;
  a.order = B->d_order;
  a.order_len = B->d_olen;
  a.order_pitch = pitch;
  a.status = B->d_si32;
  a.phase1_used = a.status + cnt;
  a.x0_slot = a.status + 2 * cnt;
  a.n_final = a.status + 3 * cnt;
  a.pivots1 = B->d_si64;
  a.pivots2 = a.pivots1 + cnt;
  a.v = B->d_sv;
  a.max_pivots = max_pivots < 0 ? -1 : max_pivots;
  a.dantzig = B->pricing == 1;
  a.fused = B->fused;
  a.lds_bytes = (int32_t)solve_launch_lds(B);
  a.threads = threads_in_effect(B, true);
  B->state = 2;
  std::vector<int32_t> h_i32(4 * cnt);
  std::vector<int64_t> h_i64(2 * cnt);
  std::vector<double> h_v(cnt);
  const double t0 = now_s();
  HIP_TRY(lpxk::launch_batch_solve(a, B->stream));
  HIP_TRY(hipStreamSynchronize(B->stream));
  const double t_pivots = now_s() - t0;
  HIP_TRY(hipMemcpyAsync(h_i32.data(), B->d_si32, h_i32.size() * sizeof(int32_t), hipMemcpyDeviceToHost, B->stream));
  HIP_TRY(hipMemcpyAsync(h_i64.data(), B->d_si64, h_i64.size() * sizeof(int64_t), hipMemcpyDeviceToHost, B->stream));
  HIP_TRY(hipMemcpyAsync(h_v.data(), B->d_sv, h_v.size() * sizeof(double), hipMemcpyDeviceToHost, B->stream));
  HIP_TRY(hipStreamSynchronize(B->stream));
  bool device_error = false;
  for (int32_t k = 0; k < count; k++) {
    lpx_solve_result& r = results[k];
    r.status = h_i32[k];
    r.phase1_used = h_i32[cnt + k];
    r.x0_slot = h_i32[2 * cnt + k];
    B->n_cur[k] = h_i32[3 * cnt + k];
    r.pivots_phase1 = h_i64[k];
    r.pivots_phase2 = h_i64[cnt + k];
    fill_objective(r, h_v[k], !maximize || maximize[k] != 0);
    device_error |= r.status == LPX_DEVICE_ERROR;
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
    const lpx_batch* B = guard.B;
    std::vector<int64_t> done(nb);
    std::vector<int32_t> st(nb);
    const double t0 = now_s();
    if (int rc = lpx_batch_simplex_loop(guard.B, o.max_pivots < 0 ? -1 : o.max_pivots, done.data(), st.data(), nullptr)) return rc;
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
    lpx_batch* B = guard.B;
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
  double* d_A = nullptr;
  int32_t cap = 0;   // scenarios the buffers below hold
  double *d_b = nullptr, *d_c = nullptr, *d_sv = nullptr, *d_x = nullptr;
  int32_t *d_flags = nullptr, *d_order = nullptr, *d_si32 = nullptr, *d_perm = nullptr;
  int64_t* d_si64 = nullptr;
  // re-solve from a shared basis (lpx_scenarios_set_basis): the eta file of the crash, the matrix and the permutation at
  // the basis; per scenario the route k_batch_resolve took
  bool has_basis = false;
  int32_t n_eta = 0;
  double *d_eta = nullptr, *d_A_basis = nullptr;
  int32_t *d_perm_basis = nullptr, *d_wanted = nullptr, *d_info = nullptr, *d_route = nullptr;
};

namespace {

void free_scenario_buffers(lpx_scenarios* S) {
  (void)hipFree(S->d_route);
  S->d_route = nullptr;
  (void)hipFree(S->d_b);
  (void)hipFree(S->d_c);
  (void)hipFree(S->d_sv);
  (void)hipFree(S->d_x);
  (void)hipFree(S->d_flags);
  (void)hipFree(S->d_si32);
  (void)hipFree(S->d_perm);
  (void)hipFree(S->d_si64);
  S->d_b = S->d_c = S->d_sv = S->d_x = nullptr;
  S->d_flags = S->d_si32 = S->d_perm = nullptr;
  S->d_si64 = nullptr;
  S->cap = 0;
}

void free_scenarios(lpx_scenarios* S) {
  if (!S) return;
  if (S->stream || S->d_A) {
    (void)hipSetDevice(S->device);
    free_scenario_buffers(S);
    (void)hipFree(S->d_A);
    (void)hipFree(S->d_order);
    (void)hipFree(S->d_eta);
    (void)hipFree(S->d_A_basis);
    (void)hipFree(S->d_perm_basis);
    (void)hipFree(S->d_wanted);
    (void)hipFree(S->d_info);
    if (S->stream) (void)hipStreamDestroy(S->stream);
  }
  delete S;
}

struct ScenariosGuard {
  lpx_scenarios* S = nullptr;
  ~ScenariosGuard() { free_scenarios(S); }
};

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

// the arguments of one solve on an m x n matrix; fills flags[count]: bit 0 = maximise, bit 1 = minInB (LPSolver.java:375-386,
// the rule of Forms::phase1) finds a negative entry in the scenario's b.  *any_p1: some scenario needs the auxiliary LP.
int check_scenario_solve(const char* who, int32_t m, int32_t n, int32_t count, const double* b, int64_t ldb, const double* c,
                         int64_t ldc, const int32_t* maximize, const int32_t* order, int32_t order_len,
                         const lpx_solve_result* results, std::vector<int32_t>& flags, bool* any_p1) {
  if (count < 0) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": negative count");
  if (ldb != 0 && ldb < m) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": ldb is neither 0 nor >= m");
  if (ldc != 0 && ldc < n) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": ldc is neither 0 nor >= n");
  if (count > 0 && !results) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": results is NULL");
  if (count > 0 && ((m > 0 && !b) || (n > 0 && !c)))
    return fail(LPX_BAD_ARGUMENT, std::string(who) + ": NULL array where data is due (b or c)");
  if (order)
    if (int rc = check_order(who, 0, m, n, order, order_len)) return rc;
  flags.assign((size_t)std::max(count, 0), 0);
  *any_p1 = false;
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
    *any_p1 |= p1;
    flags[k] = (!maximize || maximize[k] != 0 ? 1 : 0) | (p1 ? 2 : 0);
  }
  return 0;
}

int scenarios_create_checked(int32_t m, int32_t n, const double* A, int64_t lda, int device, lpx_scenarios** out) {
  ScenariosGuard guard;
  lpx_scenarios* S = guard.S = new lpx_scenarios();
  S->device = device;
  S->m = m;
  S->n = n;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreateWithFlags(&S->stream, hipStreamNonBlocking));
  HIP_TRY(hipMalloc((void**)&S->d_A, std::max<size_t>((size_t)m * n, 1) * sizeof(double)));
  HIP_TRY(hipMalloc((void**)&S->d_order, (size_t)std::max(n, 1) * sizeof(int32_t)));
  if (m > 0 && n > 0) {
    HIP_TRY(hipMemcpy2DAsync(S->d_A, (size_t)n * sizeof(double), A, (size_t)lda * sizeof(double), (size_t)n * sizeof(double),
                             (size_t)m, hipMemcpyHostToDevice, S->stream));
    HIP_TRY(hipStreamSynchronize(S->stream));   // the caller's A is free again
  }
  guard.S = nullptr;
  *out = S;
  return 0;
}

int scenarios_reserve(lpx_scenarios* S, int32_t count) {
  if (count <= S->cap) return 0;
  free_scenario_buffers(S);
  const size_t cnt = (size_t)count, m = (size_t)S->m, n = (size_t)S->n;
  HIP_TRY(hipMalloc((void**)&S->d_b, std::max<size_t>(cnt * m, 1) * sizeof(double)));
  HIP_TRY(hipMalloc((void**)&S->d_c, std::max<size_t>(cnt * n, 1) * sizeof(double)));
  HIP_TRY(hipMalloc((void**)&S->d_sv, cnt * sizeof(double)));
  HIP_TRY(hipMalloc((void**)&S->d_x, std::max<size_t>(cnt * n, 1) * sizeof(double)));
  HIP_TRY(hipMalloc((void**)&S->d_flags, cnt * sizeof(int32_t)));
  HIP_TRY(hipMalloc((void**)&S->d_si32, 4 * cnt * sizeof(int32_t)));
  HIP_TRY(hipMalloc((void**)&S->d_perm, std::max<size_t>(cnt * (n + m), 1) * sizeof(int32_t)));
  HIP_TRY(hipMalloc((void**)&S->d_si64, 2 * cnt * sizeof(int64_t)));
  HIP_TRY(hipMalloc((void**)&S->d_route, cnt * sizeof(int32_t)));
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

// the checked core of lpx_scenarios_solve: flags and any_p1 from check_scenario_solve, count > 0
int scenarios_solve_checked(const char* who, lpx_scenarios* S, int32_t count, const double* b, int64_t ldb, const double* c,
                            int64_t ldc, const std::vector<int32_t>& flags, bool any_p1, int64_t max_pivots,
                            const int32_t* restore_order, int32_t restore_order_len, lpx_solve_result* results, double* x_out,
                            int32_t* perm_out) {
  const double t_start = now_s();
  const int32_t m = S->m, n = S->n;
  std::vector<int32_t> order((size_t)std::max(n, 1), 0);
  int32_t olen = n;
  if (restore_order) {
    olen = restore_order_len < 0 ? n : restore_order_len;
    std::copy(restore_order, restore_order + olen, order.begin());
  } else if (n > 0) {
    lpx_java_default_name_order(n, order.data());
  }
  init_results(results, count);
  HIP_TRY(hipSetDevice(S->device));
  if (int rc = scenarios_reserve(S, count)) return rc;
  const size_t cnt = (size_t)count;
  if (int rc = upload_vectors(S, S->d_b, b, ldb, m, count)) return rc;
  if (int rc = upload_vectors(S, S->d_c, c, ldc, n, count)) return rc;
  HIP_TRY(hipMemcpyAsync(S->d_flags, flags.data(), cnt * sizeof(int32_t), hipMemcpyHostToDevice, S->stream));
  if (olen > 0) HIP_TRY(hipMemcpyAsync(S->d_order, order.data(), (size_t)olen * sizeof(int32_t), hipMemcpyHostToDevice, S->stream));
  lpxk::BatchScenarioArgs a{};
  a.count = count;
  a.m = m;
  a.n = n;
  a.A = S->d_A;
  a.b = S->d_b;
  a.c = S->d_c;
  a.ldb = ldb == 0 ? 0 : m;
  a.ldc = ldc == 0 ? 0 : n;
  a.flags = S->d_flags;
  a.order = S->d_order;
  a.order_len = olen;
  a.status = S->d_si32;
  a.phase1_used = a.status + cnt;
  a.x0_slot = a.status + 2 * cnt;
  a.n_final = a.status + 3 * cnt;
  a.pivots1 = S->d_si64;
  a.pivots2 = a.pivots1 + cnt;
  a.v = S->d_sv;
  a.x_out = x_out ? S->d_x : nullptr;
  a.perm_out = perm_out ? S->d_perm : nullptr;
  a.max_pivots = max_pivots < 0 ? -1 : max_pivots;
  a.dantzig = S->pricing == 1;
  a.fused = S->fused;
  a.lds_bytes = (int32_t)std::max<int64_t>(lpxk::kBatchScratchBytes, any_p1 ? solve_lds_bytes_of(m, n) : lds_bytes_of(m, n));
  a.threads = threads_or_env(threads_of(m, n + (any_p1 ? 1 : 0)));
  std::vector<int32_t> h_i32(4 * cnt);
  std::vector<int64_t> h_i64(2 * cnt);
  std::vector<double> h_v(cnt);
  HIP_TRY(hipStreamSynchronize(S->stream));   // the uploads are through: seconds_pivots is the launch alone
  const double t0 = now_s();
  HIP_TRY(lpxk::launch_batch_scenarios(a, S->stream));
  HIP_TRY(hipStreamSynchronize(S->stream));
  const double t_pivots = now_s() - t0;
  HIP_TRY(hipMemcpyAsync(h_i32.data(), S->d_si32, h_i32.size() * sizeof(int32_t), hipMemcpyDeviceToHost, S->stream));
  HIP_TRY(hipMemcpyAsync(h_i64.data(), S->d_si64, h_i64.size() * sizeof(int64_t), hipMemcpyDeviceToHost, S->stream));
  HIP_TRY(hipMemcpyAsync(h_v.data(), S->d_sv, h_v.size() * sizeof(double), hipMemcpyDeviceToHost, S->stream));
  HIP_TRY(hipStreamSynchronize(S->stream));
  bool device_error = false, all_mxn = true;
  for (int32_t k = 0; k < count; k++) {
    lpx_solve_result& r = results[k];
    r.status = h_i32[k];
    r.phase1_used = h_i32[cnt + k];
    r.x0_slot = h_i32[2 * cnt + k];
    r.pivots_phase1 = h_i64[k];
    r.pivots_phase2 = h_i64[cnt + k];
    fill_objective(r, h_v[k], (flags[k] & 1) != 0);
    device_error |= r.status == LPX_DEVICE_ERROR;
    all_mxn &= h_i32[3 * cnt + k] == n;
  }
  if (device_error) {
    stamp_seconds(results, count, t_start, t_pivots);
    return fail(LPX_DEVICE_ERROR, std::string(who) + ": the kernel and the host disagree about a scenario's layout");
  }
  // x and perm: the kernel wrote the rows of the scenarios that ended m x n and no others.  All of them (the usual
  // case): one copy each into the caller's arrays; else through a host copy, row by row
  const size_t xw = (size_t)n, pw = (size_t)n + m;
  if (all_mxn) {
    if (x_out && xw > 0) HIP_TRY(hipMemcpyAsync(x_out, S->d_x, cnt * xw * sizeof(double), hipMemcpyDeviceToHost, S->stream));
    if (perm_out && pw > 0) HIP_TRY(hipMemcpyAsync(perm_out, S->d_perm, cnt * pw * sizeof(int32_t), hipMemcpyDeviceToHost, S->stream));
    HIP_TRY(hipStreamSynchronize(S->stream));
  } else {
    std::vector<double> hx(x_out ? cnt * xw : 0);
    std::vector<int32_t> hp(perm_out ? cnt * pw : 0);
    if (!hx.empty()) HIP_TRY(hipMemcpyAsync(hx.data(), S->d_x, hx.size() * sizeof(double), hipMemcpyDeviceToHost, S->stream));
    if (!hp.empty()) HIP_TRY(hipMemcpyAsync(hp.data(), S->d_perm, hp.size() * sizeof(int32_t), hipMemcpyDeviceToHost, S->stream));
    HIP_TRY(hipStreamSynchronize(S->stream));
    for (int32_t k = 0; k < count; k++) {
      if (h_i32[3 * cnt + k] != n) continue;
      if (!hx.empty()) memcpy(x_out + k * xw, hx.data() + k * xw, xw * sizeof(double));
      if (!hp.empty()) memcpy(perm_out + k * pw, hp.data() + k * pw, pw * sizeof(int32_t));
    }
  }
  stamp_seconds(results, count, t_start, t_pivots);
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
  if (!S->d_eta) {
    const size_t etas = (size_t)std::min(m, n) * (size_t)lpxk::eta_stride(m, n);
    HIP_TRY(hipMalloc((void**)&S->d_eta, std::max<size_t>(etas, 1) * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&S->d_A_basis, std::max<size_t>((size_t)m * n, 1) * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&S->d_perm_basis, wanted.size() * sizeof(int32_t)));
    HIP_TRY(hipMalloc((void**)&S->d_wanted, wanted.size() * sizeof(int32_t)));
    HIP_TRY(hipMalloc((void**)&S->d_info, 2 * sizeof(int32_t)));
  }
  HIP_TRY(hipMemcpyAsync(S->d_wanted, wanted.data(), wanted.size() * sizeof(int32_t), hipMemcpyHostToDevice, S->stream));
  lpxk::ScenarioCrashArgs a{};
  a.count = 1;
  a.m = m;
  a.n = n;
  a.A = S->d_A;
  a.wanted = S->d_wanted;
  a.A_out = S->d_A_basis;
  a.perm_out = S->d_perm_basis;
  a.eta = S->d_eta;
  a.info = S->d_info;
  a.fused = S->fused;
  a.lds_bytes = (int32_t)std::max<int64_t>(lpxk::kBatchScratchBytes, lds_bytes_of(m, n));
  a.threads = threads_or_env(threads_of(m, n));
  HIP_TRY(lpxk::launch_scenarios_crash(a, S->stream));
  int32_t info[2] = {0, -2};
  HIP_TRY(hipMemcpyAsync(info, S->d_info, sizeof info, hipMemcpyDeviceToHost, S->stream));
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

// the checked core of lpx_scenarios_resolve: flags from check_scenario_solve, count > 0, the handle has a basis
int scenarios_resolve_checked(const char* who, lpx_scenarios* S, int32_t count, const double* b, int64_t ldb, const double* c,
                              int64_t ldc, const std::vector<int32_t>& flags, int64_t max_pivots, const int32_t* restore_order,
                              int32_t restore_order_len, lpx_solve_result* results, double* x_out, int32_t* perm_out,
                              int32_t* route_out) {
  const double t_start = now_s();
  const int32_t m = S->m, n = S->n;
  init_results(results, count);
  HIP_TRY(hipSetDevice(S->device));
  if (int rc = scenarios_reserve(S, count)) return rc;
  const size_t cnt = (size_t)count;
  if (int rc = upload_vectors(S, S->d_b, b, ldb, m, count)) return rc;
  if (int rc = upload_vectors(S, S->d_c, c, ldc, n, count)) return rc;
  HIP_TRY(hipMemcpyAsync(S->d_flags, flags.data(), cnt * sizeof(int32_t), hipMemcpyHostToDevice, S->stream));
  lpxk::BatchResolveArgs a{};
  a.count = count;
  a.m = m;
  a.n = n;
  a.A = S->d_A_basis;
  a.b = S->d_b;
  a.c = S->d_c;
  a.ldb = ldb == 0 ? 0 : m;
  a.ldc = ldc == 0 ? 0 : n;
  a.flags = S->d_flags;
  a.status = S->d_si32;
  a.phase1_used = a.status + cnt;
  a.x0_slot = a.status + 2 * cnt;
  a.n_final = a.status + 3 * cnt;
  a.pivots1 = S->d_si64;
  a.pivots2 = a.pivots1 + cnt;
  a.v = S->d_sv;
  a.x_out = x_out ? S->d_x : nullptr;
  a.perm_out = perm_out ? S->d_perm : nullptr;
  a.max_pivots = max_pivots < 0 ? -1 : max_pivots;
  a.dantzig = S->pricing == 1;
  a.fused = S->fused;
  a.lds_bytes = (int32_t)std::max<int64_t>(lpxk::kBatchScratchBytes, lds_bytes_of(m, n));
  a.threads = threads_or_env(threads_of(m, n));
  a.perm0 = S->d_perm_basis;
  a.eta = S->d_eta;
  a.n_eta = S->n_eta;
  a.route = S->d_route;
  std::vector<int32_t> h_route(cnt), h_i32(4 * cnt);
  std::vector<int64_t> h_i64(2 * cnt);
  std::vector<double> h_v(cnt);
  HIP_TRY(hipStreamSynchronize(S->stream));   // the uploads are through: seconds_pivots is the launches alone
  const double t0 = now_s();
  HIP_TRY(lpxk::launch_batch_resolve(a, S->stream));
  HIP_TRY(hipStreamSynchronize(S->stream));
  double t_pivots = now_s() - t0;
  HIP_TRY(hipMemcpyAsync(h_route.data(), S->d_route, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, S->stream));
  HIP_TRY(hipMemcpyAsync(h_i32.data(), S->d_si32, h_i32.size() * sizeof(int32_t), hipMemcpyDeviceToHost, S->stream));
  HIP_TRY(hipMemcpyAsync(h_i64.data(), S->d_si64, h_i64.size() * sizeof(int64_t), hipMemcpyDeviceToHost, S->stream));
  HIP_TRY(hipMemcpyAsync(h_v.data(), S->d_sv, h_v.size() * sizeof(double), hipMemcpyDeviceToHost, S->stream));
  HIP_TRY(hipStreamSynchronize(S->stream));
  std::vector<int32_t> cold;
  bool device_error = false;
  for (int32_t k = 0; k < count; k++) {
    if (h_route[k] == LPX_ROUTE_COLD) {
      cold.push_back(k);
      continue;
    }
    lpx_solve_result& r = results[k];
    r.status = h_i32[k];
    r.phase1_used = 0;
    r.x0_slot = -1;
    r.pivots_phase1 = h_i64[k];
    r.pivots_phase2 = h_i64[cnt + k];
    fill_objective(r, h_v[k], (flags[k] & 1) != 0);
    device_error |= r.status == LPX_DEVICE_ERROR;
  }
  if (device_error) {
    stamp_seconds(results, count, t_start, t_pivots);
    return fail(LPX_DEVICE_ERROR, std::string(who) + ": the kernel and the host disagree about a scenario's layout");
  }
  // x and perm of the warm scenarios (their final state is always m x n): all of them, one copy each into the caller's
  // arrays; else through a host copy, row by row -- the cold solve below reuses the device rows
  const size_t xw = (size_t)n, pw = (size_t)n + m;
  if (cold.empty()) {
    if (x_out && xw > 0) HIP_TRY(hipMemcpyAsync(x_out, S->d_x, cnt * xw * sizeof(double), hipMemcpyDeviceToHost, S->stream));
    if (perm_out && pw > 0) HIP_TRY(hipMemcpyAsync(perm_out, S->d_perm, cnt * pw * sizeof(int32_t), hipMemcpyDeviceToHost, S->stream));
    HIP_TRY(hipStreamSynchronize(S->stream));
  } else {
    std::vector<double> hx(x_out ? cnt * xw : 0);
    std::vector<int32_t> hp(perm_out ? cnt * pw : 0);
    if (!hx.empty()) HIP_TRY(hipMemcpyAsync(hx.data(), S->d_x, hx.size() * sizeof(double), hipMemcpyDeviceToHost, S->stream));
    if (!hp.empty()) HIP_TRY(hipMemcpyAsync(hp.data(), S->d_perm, hp.size() * sizeof(int32_t), hipMemcpyDeviceToHost, S->stream));
    HIP_TRY(hipStreamSynchronize(S->stream));
    for (int32_t k = 0; k < count; k++) {
      if (h_route[k] == LPX_ROUTE_COLD) continue;
      if (!hx.empty()) memcpy(x_out + k * xw, hx.data() + k * xw, xw * sizeof(double));
      if (!hp.empty()) memcpy(perm_out + k * pw, hp.data() + k * pw, pw * sizeof(int32_t));
    }
    // the cold scenarios: lpx_scenarios_solve on their rows of b and c, gathered; results, x and perm scattered back
    const int32_t nc = (int32_t)cold.size();
    std::vector<double> gb(ldb == 0 ? 0 : (size_t)nc * m), gc(ldc == 0 ? 0 : (size_t)nc * n);
    std::vector<int32_t> gflags(nc);
    bool any_p1 = false;
    for (int32_t t = 0; t < nc; t++) {
      const int32_t k = cold[t];
      if (ldb != 0 && m > 0) memcpy(&gb[(size_t)t * m], b + k * ldb, (size_t)m * sizeof(double));
      if (ldc != 0 && n > 0) memcpy(&gc[(size_t)t * n], c + k * ldc, (size_t)n * sizeof(double));
      gflags[t] = flags[k];
      any_p1 |= (flags[k] & 2) != 0;
    }
    std::vector<lpx_solve_result> res(nc);
    std::vector<double> tx(x_out ? (size_t)nc * xw : 0);
    std::vector<int32_t> tp((size_t)nc * pw, -1);   // a row the solve leaves alone (ended inside phase 1) still starts with -1
    if (int rc = scenarios_solve_checked(who, S, nc, ldb == 0 ? b : gb.data(), ldb == 0 ? 0 : m, ldc == 0 ? c : gc.data(),
                                         ldc == 0 ? 0 : n, gflags, any_p1, max_pivots, restore_order, restore_order_len,
                                         res.data(), tx.empty() ? nullptr : tx.data(), tp.empty() ? nullptr : tp.data()))
      return rc;
    t_pivots += res[0].seconds_pivots;
    for (int32_t t = 0; t < nc; t++) {
      const int32_t k = cold[t];
      results[k] = res[t];
      if (pw > 0 && tp[(size_t)t * pw] < 0) continue;
      if (!tx.empty()) memcpy(x_out + k * xw, tx.data() + t * xw, xw * sizeof(double));
      if (perm_out && pw > 0) memcpy(perm_out + k * pw, tp.data() + t * pw, pw * sizeof(int32_t));
    }
  }
  if (route_out) memcpy(route_out, h_route.data(), cnt * sizeof(int32_t));
  stamp_seconds(results, count, t_start, t_pivots);
  return 0;
}

}  // namespace

extern "C" int lpx_scenarios_create(int32_t m, int32_t n, const double* A, int64_t lda, int device, lpx_scenarios** out) {
  if (!out) return fail(LPX_BAD_ARGUMENT, "lpx_scenarios_create: out is NULL");
  *out = nullptr;
  if (int rc = check_scenario_matrix("lpx_scenarios_create", m, n, A, lda, device)) return rc;
  DeviceRestore keep_device;
  return scenarios_create_checked(m, n, A, lda, device, out);
}

extern "C" void lpx_scenarios_destroy(lpx_scenarios* S) {
  DeviceRestore keep_device;
  free_scenarios(S);
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
  std::vector<int32_t> flags;
  bool any_p1 = false;
  if (int rc = check_scenario_solve(who, S->m, S->n, count, b, ldb, c, ldc, maximize, restore_order, restore_order_len, results,
                                    flags, &any_p1))
    return rc;
  if (count == 0) return 0;
  DeviceRestore keep_device;
  return scenarios_solve_checked(who, S, count, b, ldb, c, ldc, flags, any_p1, max_pivots, restore_order, restore_order_len,
                                 results, x_out, perm_out);
}

// create, solve, destroy
extern "C" int lpx_solve_scenarios(int32_t m, int32_t n, const double* A, int64_t lda, int32_t count, const double* b,
                                   int64_t ldb, const double* c, int64_t ldc, const int32_t* maximize,
                                   const lpx_solve_options* opts, lpx_solve_result* results, double* x_out, int32_t* perm_out) {
  const char* who = "lpx_solve_scenarios";
  lpx_solve_options o{};
  o.max_pivots = -1;
  if (opts) o = *opts;
  if (o.keep_state || o.perm_out || o.x_out)
    return fail(LPX_BAD_ARGUMENT, std::string(who) + ": opts->keep_state, opts->perm_out and opts->x_out must be NULL");
  if (o.pricing != 0 && o.pricing != 1) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": bad pricing");
  if (int rc = check_scenario_matrix(who, m, n, A, lda, o.device)) return rc;
  std::vector<int32_t> flags;
  bool any_p1 = false;
  if (int rc = check_scenario_solve(who, m, n, count, b, ldb, c, ldc, maximize, o.restore_order, o.restore_order_len, results,
                                    flags, &any_p1))
    return rc;
  if (count == 0) return 0;
  const double t_start = now_s();
  DeviceRestore keep_device;
  ScenariosGuard guard;
  if (int rc = scenarios_create_checked(m, n, A, lda, o.device, &guard.S)) return rc;
  guard.S->fused = o.fused > 0;   // 0 = the library's choice by size = two roundings here, as in lpx_solve at these sizes
  guard.S->pricing = o.pricing;
  if (int rc = scenarios_solve_checked(who, guard.S, count, b, ldb, c, ldc, flags, any_p1, o.max_pivots, o.restore_order,
                                       o.restore_order_len, results, x_out, perm_out))
    return rc;
  stamp_seconds(results, count, t_start, results[0].seconds_pivots);   // the times of the whole call, creation included
  return 0;
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
  std::vector<int32_t> flags;
  bool any_p1 = false;
  if (int rc = check_scenario_solve(who, S->m, S->n, count, b, ldb, c, ldc, maximize, restore_order, restore_order_len, results,
                                    flags, &any_p1))
    return rc;
  if (!S->has_basis) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": the handle has no basis (lpx_scenarios_set_basis)");
  if (count == 0) return 0;
  DeviceRestore keep_device;
  return scenarios_resolve_checked(who, S, count, b, ldb, c, ldc, flags, max_pivots, restore_order, restore_order_len, results,
                                   x_out, perm_out, route_out);
}

// create, set_basis, resolve, destroy
extern "C" int lpx_solve_scenarios_from_basis(int32_t m, int32_t n, const double* A, int64_t lda, const int32_t* basis,
                                              int32_t count, const double* b, int64_t ldb, const double* c, int64_t ldc,
                                              const int32_t* maximize, const lpx_solve_options* opts, lpx_solve_result* results,
                                              double* x_out, int32_t* perm_out, int32_t* route_out) {
  const char* who = "lpx_solve_scenarios_from_basis";
  lpx_solve_options o{};
  o.max_pivots = -1;
  if (opts) o = *opts;
  if (o.keep_state || o.perm_out || o.x_out)
    return fail(LPX_BAD_ARGUMENT, std::string(who) + ": opts->keep_state, opts->perm_out and opts->x_out must be NULL");
  if (o.pricing != 0 && o.pricing != 1) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": bad pricing");
  if (int rc = check_scenario_matrix(who, m, n, A, lda, o.device)) return rc;
  if (!basis) return fail(LPX_BAD_ARGUMENT, std::string(who) + ": basis is NULL");
  if (int rc = check_basis(who, m, n, basis)) return rc;
  std::vector<int32_t> flags;
  bool any_p1 = false;
  if (int rc = check_scenario_solve(who, m, n, count, b, ldb, c, ldc, maximize, o.restore_order, o.restore_order_len, results,
                                    flags, &any_p1))
    return rc;
  if (count == 0) return 0;
  const double t_start = now_s();
  DeviceRestore keep_device;
  ScenariosGuard guard;
  if (int rc = scenarios_create_checked(m, n, A, lda, o.device, &guard.S)) return rc;
  guard.S->fused = o.fused > 0;   // 0 = the library's choice by size = two roundings here, as in lpx_solve at these sizes
  guard.S->pricing = o.pricing;
  if (int rc = scenarios_set_basis_checked(who, guard.S, basis, nullptr)) return rc;
  if (int rc = scenarios_resolve_checked(who, guard.S, count, b, ldb, c, ldc, flags, o.max_pivots, o.restore_order,
                                         o.restore_order_len, results, x_out, perm_out, route_out))
    return rc;
  stamp_seconds(results, count, t_start, results[0].seconds_pivots);   // the times of the whole call, creation and crash included
  return 0;
}

// What the launch of lpx_scenarios_resolve looks like for this handle, and the entries of its eta file
// (scripts/bench_scenarios_resolve.py): not part of include/lpx.h
extern "C" int lpxi_scenarios_resolve_launch_info(lpx_scenarios* S, int32_t* threads, int32_t* lds_bytes, int32_t* blocks_per_cu,
                                                  int32_t* etas) {
  if (!S) return fail(LPX_BAD_ARGUMENT, "lpxi_scenarios_resolve_launch_info: NULL handle");
  DeviceRestore keep_device;
  HIP_TRY(hipSetDevice(S->device));
  const int t = threads_or_env(threads_of(S->m, S->n));
  const int lds = (int)std::min<int64_t>(std::max<int64_t>(lpxk::kBatchScratchBytes, lds_bytes_of(S->m, S->n)), INT32_MAX);
  if (threads) *threads = t;
  if (lds_bytes) *lds_bytes = lds;
  if (blocks_per_cu) *blocks_per_cu = lpxk::batch_resolve_blocks_per_cu(t, lds);
  if (etas) *etas = S->has_basis ? S->n_eta : -1;
  return 0;
}

// What the launch of lpx_scenarios_solve looks like for this handle (scripts/bench_scenarios.py): not part of include/lpx.h
extern "C" int lpxi_scenarios_launch_info(lpx_scenarios* S, int32_t phase1, int32_t* threads, int32_t* lds_bytes,
                                          int32_t* blocks_per_cu) {
  if (!S) return fail(LPX_BAD_ARGUMENT, "lpxi_scenarios_launch_info: NULL handle");
  DeviceRestore keep_device;
  HIP_TRY(hipSetDevice(S->device));
  const int t = threads_or_env(threads_of(S->m, S->n + (phase1 ? 1 : 0)));
  const int lds = (int)std::min<int64_t>(std::max<int64_t>(lpxk::kBatchScratchBytes, phase1 ? solve_lds_bytes_of(S->m, S->n)
                                                                                            : lds_bytes_of(S->m, S->n)), INT32_MAX);
  if (threads) *threads = t;
  if (lds_bytes) *lds_bytes = lds;
  if (blocks_per_cu) *blocks_per_cu = lpxk::batch_scenarios_blocks_per_cu(t, lds);
  return 0;
}
