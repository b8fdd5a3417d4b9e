// api.hip -- the C ABI (include/gtsam_amd.h): handle life cycle, the per-iteration entry points (linearize / try_lambda / accept)
// that issue the HIP kernels, getters and test hooks.  The upload of the factor tables (shard filter, noise table) is upload.hip,
// the one-time symbolic analysis of a graph analysis.hip, what a handle owns on its device and how it is released
// device_memory.hip.  All arithmetic of the hot path runs in the HIP kernels.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <set>
#include <memory>
#include <mutex>
#include <stdexcept>

#include "analysis.h"
#include "factors.h"
#include "kernels.h"

namespace gt {

// gtg_prewarm's registry (kernels.h): filled by the static PrewarmUnit objects of the translation units
static std::vector<void (*)(int)>& prewarm_units() { static std::vector<void (*)(int)> v; return v; }
PrewarmUnit::PrewarmUnit(void (*fn)(int device)) { prewarm_units().push_back(fn); }

static thread_local std::string g_last_error;

static void exchange(gtg_context& c, double* ptr, int64_t n);
void exchange_sum(gtg_context& c, double* ptr, int64_t n) { exchange(c, ptr, n); }
static void exchange(gtg_context& c, double* ptr, int64_t n) {
  if (c.n_shards > 1) {
    if (!c.allreduce) throw std::runtime_error("n_shards > 1 but no allreduce callback was set (gtg_set_allreduce)");
    if (!c.layout_verified) verify_layout(c);   // the callback was registered after the upload
    const int rc = c.allreduce(ptr, n, (void*)c.stream, c.allreduce_user);
    if (rc != 0) throw std::runtime_error("allreduce callback failed");
  }
}

// The dataflow factorisation is a pair of persistent kernels that wait for each other.  Two of them in flight on one device (two
// handles driven from two host threads) can starve each other: the runtime multiplexes streams onto a few hardware queues, and
// handle A's chain kernel may sit behind handle B's bulk kernel in one queue while B's chain kernel sits behind A's bulk kernel
// in another -- neither pair completes until the wait bound breaks the cycle (seen with three handles: time-outs, never wrong
// numbers).  So a process runs one dataflow factorisation per device at a time: the lock is taken before the launch and released
// once the call has synchronised with its stream.
static std::mutex& df_device_lock(int device) {
  static std::mutex guard;
  static std::map<int, std::unique_ptr<std::mutex>> locks;
  std::lock_guard<std::mutex> g(guard);
  auto& p = locks[device];
  if (!p) p.reset(new std::mutex);
  return *p;
}

// Sharded: the scalars are partial sums and get all-reduced -- a COPY of them (second half of the buffer), so that slots a call
// does not rewrite are not multiplied by the number of shards on every call (they would overflow to inf after a few hundred).
static void read_scalars(gtg_context& c) {
  const double* src = c.scalars.p;
  if (c.n_shards > 1) {
    check_hip(hipMemcpyAsync(c.scalars.p + SC_COUNT, c.scalars.p, sizeof(double) * SC_COUNT, hipMemcpyDeviceToDevice, c.stream), "D2D");
    exchange(c, c.scalars.p + SC_COUNT, SC_COUNT);
    src = c.scalars.p + SC_COUNT;
  }
  check_hip(hipMemcpyAsync(c.h_scalars, src, sizeof(double) * SC_COUNT, hipMemcpyDeviceToHost, c.stream), "D2H");
  check_hip(hipStreamSynchronize(c.stream), "sync");
  c.h_scalars[SC_DELTA_SQ] /= c.n_shards;  // identical on every shard, summed by the exchange
}

// The kernels that follow LM's "is the linear cost change >= 0" (LevenbergMarquardtOptimizer.cpp:180-191: no error evaluation, hence no
// re-triangulation, of a trial step the model does not like) read the two linear errors on the device.  On a sharded graph every shard
// holds only its share of them: the sums are exchanged first, into a copy (read_scalars sums the originals once more, later).
static bool smart_gate(gtg_context& c) {
  if (!c.n_smart || c.n_shards == 1) return false;
  check_hip(hipMemcpyAsync(c.scalars.p + 2 * SC_COUNT, c.scalars.p, sizeof(double) * SC_COUNT, hipMemcpyDeviceToDevice, c.stream), "D2D");
  exchange(c, c.scalars.p + 2 * SC_COUNT, SC_COUNT);
  return true;
}

static void check_smart_supported(gtg_context& c, const char* where) {
  if (!c.n_smart || c.h_scalars[SC_UNSUPPORTED] == 0.0) return;
  // the two places where the reference's smart factor throws out of linearize() / error() instead of returning a number
  if (c.h_scalars[SC_UNSUPPORTED] >= kUnsupportedCheirality)      // (summed over the shards: calibrate counts 1 per shard)
    throw std::runtime_error(std::string(where) + ": CheiralityException -- a smart factor's point at infinity (IGNORE_DEGENERACY / HANDLE_INFINITY "
                             "with a landmark that did not triangulate) lies behind one of the factor's cameras, or the refinement of a "
                             "triangulation (enableEPI) linearised at a point behind a camera; the reference throws here");
  throw std::runtime_error(std::string(where) + ": Cal3Bundler::calibrate did not converge for a measurement of a smart factor; the reference throws here");
}

struct PhaseTimer {
  gtg_context& c; int ph; hipEvent_t a, b;
  PhaseTimer(gtg_context& c_, int ph_) : c(c_), ph(ph_), a(c_.phase_events[2 * ph_]), b(c_.phase_events[2 * ph_ + 1]) {
    if (c.timing) (void)hipEventRecord(a, c.stream);
  }
  ~PhaseTimer() { if (c.timing) (void)hipEventRecord(b, c.stream); }
};
static void ensure_events(gtg_context& c) {   // the handle's own events, on its device
  if (!c.phase_events.empty()) return;
  c.phase_events.resize(2 * GTG_PH_COUNT, nullptr);
  for (auto& e : c.phase_events) check_hip(hipEventCreate(&e), "event");
}
static void collect(gtg_context& c, std::initializer_list<int> phases) {
  if (!c.timing) return;
  for (int ph : phases) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, c.phase_events[2 * ph], c.phase_events[2 * ph + 1]) == hipSuccess) { c.phase_ms[ph] += ms; c.phase_calls[ph]++; }
  }
}

}  // namespace gt

namespace gt { long long* g_potrf_dbg_set(long long*); float debug_time_syrk(gtg_context&, SMat, int, int, int); }
using namespace gt;

#define GTG_TRY try {
#define GTG_CATCH                                                                     \
  } catch (const std::invalid_argument& e) { g_last_error = e.what(); return GTG_ERR_USAGE; } \
  catch (const std::exception& e) { g_last_error = e.what(); return GTG_ERR_HIP; }

extern "C" {

const char* gtg_last_error(void) { return g_last_error.c_str(); }
const char* gtg_version(void) { return "gtsam_amd 0.1 (gfx950, FP64)"; }
const char* gtg_phase_name(int ph) {
  static const char* names[GTG_PH_COUNT] = {"linearize", "assemble", "point_eliminate", "schur", "cholesky",
                                            "solve", "linear_error", "retract", "error"};
  return (ph >= 0 && ph < GTG_PH_COUNT) ? names[ph] : "?";
}

int gtg_create(gtg_handle* out, int device_id) {
  GTG_TRY
  if (!out) throw std::invalid_argument("null out");
  int ndev = 0;
  check_hip(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
  if (device_id < 0 || device_id >= ndev) throw std::invalid_argument("bad device id (no HIP device visible?)");
  check_hip(hipSetDevice(device_id), "hipSetDevice");
  gtg_context* c = new gtg_context;
  c->device = device_id;
  if (!take_parked(*c)) {
    check_hip(hipStreamCreate(&c->stream), "hipStreamCreate");
    check_hip(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking), "hipStreamCreate");   // uploads beside the analysis (gtg_upload_problem)
    ensure_events(*c);
  }
  *out = c;
  return GTG_OK;
  GTG_CATCH
}

// The one-time work of a process on a device, done ahead of the first handle: runtime start and device context, the code objects of
// the library's translation units and the function objects of their kernels (every unit registers its list, kernels.h), the default
// pair of CU-masked streams of the dataflow factorisation, a first stream / event.  Idempotent per device; safe to call from a helper
// thread while the caller prepares its problem (the C++ shim's constructor does: GpuLevenbergMarquardtOptimizer.cpp).
int gtg_prewarm(int device_id) {
  GTG_TRY
  static std::mutex mu;
  static std::set<int> done;
  std::lock_guard<std::mutex> lock(mu);
  if (done.count(device_id)) return GTG_OK;
  int ndev = 0;
  check_hip(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
  if (device_id < 0 || device_id >= ndev) throw std::invalid_argument("bad device id (no HIP device visible?)");
  check_hip(hipSetDevice(device_id), "hipSetDevice");
  (void)hipFree(nullptr);
  hipStream_t st = nullptr; hipEvent_t ev = nullptr;
  check_hip(hipStreamCreate(&st), "hipStreamCreate");
  check_hip(hipEventCreate(&ev), "hipEventCreate");
  for (auto fn : prewarm_units()) fn(device_id);
  (void)hipEventRecord(ev, st);
  (void)hipStreamSynchronize(st);
  (void)hipEventDestroy(ev);
  (void)hipStreamDestroy(st);
  done.insert(device_id);
  return GTG_OK;
  GTG_CATCH
}

int gtg_destroy(gtg_handle c) {
  if (!c) return GTG_OK;
  try { join_block_level(*c); } catch (...) {}
  try { df_join_prepared(); } catch (...) {}
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  // The releases below run while no dataflow factorisation of ANOTHER handle is in flight on this device: a handle that was destroyed
  // beside a running factorisation stalled its persistent kernels past the 20 ms bound of their dependency waits (three of three time-outs of
  // the round's last multi-handle stress runs sat in the second-to-last factorisation of a handle whose neighbour had just finished:
  // profiles/r06_stress_240s.txt).  GTG_DESTROY_UNLOCKED=1: the A/B.
  std::unique_lock<std::mutex> no_factorisation_in_flight;
  if (!std::getenv("GTG_DESTROY_UNLOCKED")) no_factorisation_in_flight = std::unique_lock<std::mutex>(df_device_lock(c->device));
  // What outlives the handle -- its stream, copy stream and phase events -- is taken out of it; everything else it owns (all its device
  // memory, the schedule's streams and events, the host index) goes with the context: here, under the lock, on the handle's device,
  // before the streams are parked.
  ParkedQueue q{c->device, c->stream, c->copy_stream, std::move(c->phase_events)};
  delete c;
  if (q.copy_stream) (void)hipStreamSynchronize(q.copy_stream);
  if (!park_queue(q)) {
    for (hipEvent_t e : q.events) if (e) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(q.stream);
    if (q.copy_stream) (void)hipStreamDestroy(q.copy_stream);
  }
  return GTG_OK;
}

int gtg_upload_problem(gtg_handle c, const gtg_problem* p_user, int shard, int n_shards) {
  GTG_TRY
  if (!c || !p_user) throw std::invalid_argument("null argument");
  if (n_shards < 1 || shard < 0 || shard >= n_shards) throw std::invalid_argument("bad shard / n_shards");
  DeviceGuard on_device(c->device);
  upload_problem(*c, *p_user, shard, n_shards);
  c->uploaded = true; c->linearized = false; c->have_trial = false;
  return GTG_OK;
  GTG_CATCH
}

int gtg_set_reduced_ordering(gtg_handle c, const int32_t* order, int32_t n) {
  GTG_TRY
  if (!c) throw std::invalid_argument("null handle");
  HostIndex& hi = host_index(c);
  hi.user_order.assign(order, order + n);
  if (c->uploaded) { check_hip(hipSetDevice(c->device), "hipSetDevice"); analyze(*c); c->linearized = false; c->have_trial = false; }
  return GTG_OK;
  GTG_CATCH
}

// The camera model of every calib row of the NEXT upload (upload.hip::take_calibration_models checks it against that problem, uses it
// and clears it): kept in the host index like the reduced ordering, because gtg_problem has no field for it.
int gtg_set_calibration_models(gtg_handle c, const int32_t* model, int32_t n_calib) {
  GTG_TRY
  if (!c) throw std::invalid_argument("null handle");
  if (n_calib < 0) throw std::invalid_argument("gtg_set_calibration_models: n_calib is negative");
  HostIndex& hi = host_index(c);
  if (!model || n_calib == 0) hi.calib_model.clear();
  else hi.calib_model.assign(model, model + n_calib);
  return GTG_OK;
  GTG_CATCH
}

int64_t gtg_values_size(gtg_handle c) { return c ? c->user_val_size : -1; }
int64_t gtg_tangent_size(gtg_handle c) { return c ? c->user_dim_size : -1; }
int64_t gtg_reduced_dim(gtg_handle c) { return c ? c->n_red : -1; }

int gtg_set_values(gtg_handle c, const double* packed, int64_t n) {
  GTG_TRY
  if (!c || !c->uploaded || n != c->user_val_size) throw std::invalid_argument("gtg_set_values: wrong size or no problem uploaded");
  DeviceGuard on_device(c->device);
  check_hip(hipMemcpyAsync(c->values.p, packed, sizeof(double) * n, hipMemcpyHostToDevice, c->stream), "H2D");
  check_hip(hipStreamSynchronize(c->stream), "sync");
  c->linearized = false; c->have_trial = false;
  return GTG_OK;
  GTG_CATCH
}

static int get_buf(gtg_handle c, const double* dev, int64_t have, double* out, int64_t n) {
  GTG_TRY
  if (!c || !c->uploaded || n != have) throw std::invalid_argument("getter: wrong size or no problem uploaded");
  DeviceGuard on_device(c->device);
  check_hip(hipMemcpyAsync(out, dev, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream), "D2H");
  check_hip(hipStreamSynchronize(c->stream), "sync");
  return GTG_OK;
  GTG_CATCH
}
int gtg_get_values(gtg_handle c, double* packed, int64_t n) { return get_buf(c, c ? c->values.p : nullptr, c ? c->user_val_size : -1, packed, n); }
int gtg_get_trial_values(gtg_handle c, double* packed, int64_t n) { return get_buf(c, c ? c->trial.p : nullptr, c ? c->user_val_size : -1, packed, n); }
int gtg_get_delta(gtg_handle c, double* d, int64_t n) { return get_buf(c, c ? c->delta.p : nullptr, c ? c->user_dim_size : -1, d, n); }

int gtg_error(gtg_handle c, double* error) {
  GTG_TRY
  if (!c || !c->uploaded || !error) throw std::invalid_argument("gtg_error: no problem uploaded");
  DeviceGuard on_device(c->device);
  if (c->n_smart) check_hip(hipMemsetAsync(c->scalars.p + SC_UNSUPPORTED, 0, sizeof(double), c->stream), "memset");
  { PhaseTimer t(*c, GTG_PH_ERROR); launch_smart_triangulate(*c, c->values.p, nullptr, false); launch_error(*c, c->values.p, SC_ERROR); }
  read_scalars(*c);
  collect(*c, {GTG_PH_ERROR});
  check_smart_supported(*c, "gtg_error");
  *error = c->h_scalars[SC_ERROR];
  return GTG_OK;
  GTG_CATCH
}

// GTG_DEBUG_TIMING=1: the host time of every phase of the FIRST linearisation and the FIRST lambda try of the process, each behind a stream
// synchronisation -- what a cold process pays there once (40 - 50 ms on the L1723 shape against 6 ms for every later iteration).
struct FirstCallClock {
  bool on; hipStream_t s; std::chrono::high_resolution_clock::time_point t;
  FirstCallClock(std::atomic<int>& calls, hipStream_t stream) : on(std::getenv("GTG_DEBUG_TIMING") != nullptr && calls.fetch_add(1) == 0), s(stream), t(std::chrono::high_resolution_clock::now()) {}
  void lap(const char* what) {
    if (!on) return;
    (void)hipStreamSynchronize(s);
    const auto n = std::chrono::high_resolution_clock::now();
    std::fprintf(stderr, "[gtsam_amd first ] %-40s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
    t = n;
  }
};
static std::atomic<int> g_first_linearize{0}, g_first_try{0};

// ---- the pieces gtg_try_lambda and gtg_try_lambda_pcg are made of ------------------------------------------------------------
// Sharded: the one big exchange, reduced Hessian + rhs summed over the shards in place
static void exchange_reduced_system(gtg_context& c) {
  if (c.n_shards == 1) return;
  if (c.n_xb == 0) {     // (no block list: whole stored 128x128 tiles, the first version of the exchange)
    const int64_t nb = c.plan.n_exch * kTile * kTile;
    if ((int64_t)c.xbuf.n != nb) c.xbuf.alloc(nb);
    launch_pack_tiles(c, smat(c), c.plan, c.xbuf.p, false);
    exchange(c, c.xbuf.p, nb);
    launch_pack_tiles(c, smat(c), c.plan, c.xbuf.p, true);
  } else {                // only the structurally non-zero d x d blocks (the same list on every shard) + rhs row + padding
    const int64_t nb = exchange_block_doubles(c);
    if ((int64_t)c.xbuf.n != nb) c.xbuf.alloc(nb);
    launch_pack_blocks(c, smat(c), c.NP, c.xbuf.p, false);
    exchange(c, c.xbuf.p, nb);
    launch_pack_blocks(c, smat(c), c.NP, c.xbuf.p, true);
  }
}

// post-mortem of a try (number `attempt`, dataflow schedule or not) that is about to be repeated: which wait gave up
// (chol_dataflow.hip::wait_flags records the first one of a dataflow pass), what it saw, and what the same words hold in memory NOW,
// read from the host after the kernels have drained.  GTG_QUIET: nothing
static void report_wait_timeout(gtg_context& c, bool df, int attempt) {
  static const bool quiet = std::getenv("GTG_QUIET") != nullptr;
  if (quiet) return;
  int32_t ctl[16] = {0};
  long long now1 = -1, now2 = -1;
  const int nt = c.NP / kTile;
  if (df && c.df.ctrl.p) {
    (void)hipMemcpy(ctl, c.df.ctrl.p, sizeof(ctl), hipMemcpyDeviceToHost);
    const int kind = ctl[8], I = ctl[9], J = ctl[10], k = ctl[11];
    const long long *w1 = nullptr, *w2 = nullptr;
    // (flag words are indexed by tile slot; kinds 1 / 2 record the SLOT of the first operand tile in k)
    auto slot_of = [&](int a, int b) { return (a >= 0 && a <= nt && b >= 0 && b < nt) ? (int64_t)c.plan.h_slot[(size_t)a * nt + b] : (int64_t)-1; };
    if (kind == 1 || kind == 2) { if (k >= 0 && k < c.plan.n_stored) w1 = w2 = c.df.tile_flag.p + k; }
    else if (kind == 3 && slot_of(J, J) >= 0) w1 = w2 = c.df.tile_flag.p + slot_of(J, J);
    else if (kind == 4) w1 = w2 = c.df.pd_flag.p + I;
    else if (kind == 5 && slot_of(I, J) >= 0) w1 = w2 = c.df.tile_flag.p + slot_of(I, J);
    else if (kind == 7 && slot_of(I, J) >= 0) w1 = w2 = c.df.part_flag.p + slot_of(I, J);
    if (w1) { (void)hipMemcpy(&now1, w1, 8, hipMemcpyDeviceToHost); (void)hipMemcpy(&now2, w2, 8, hipMemcpyDeviceToHost); }
  }
  std::fprintf(stderr, "[gtsam_amd] %s factorisation (epoch %lld): a dependency wait ran into its bound; repeating the lambda try with the %s "
               "schedule.  wait kind %d at (%d, %d, %d): saw %d / %d, wanted %d / %d; memory now holds %lld / %lld; waiter on XCD %d (hw id 0x%x); "
               "tickets taken %d, diagonal tiles started %d of %d; over this handle's life: waits that ended on the shadow words %d, on the read-modify-write poll %d\n",
               df ? "dataflow" : "stream-schedule", c.chol_epoch, (c.use_df && attempt + 1 != 2) ? "dataflow" : "stream", ctl[8], ctl[9], ctl[10], ctl[11], ctl[12], ctl[13], ctl[14],
               ctl[15], now1, now2, ctl[2], (unsigned)ctl[3], ctl[0], ctl[1], nt, ctl[6], ctl[7]);
}

// end of either solve: the landmarks' steps (sharded: every landmark's from the shard that owns it) into the step of all variables
static void scatter_step(gtg_context& c) {
  if (c.n_lm) exchange(c, c.delta_lm.p, 3 * (int64_t)c.n_lm);
  launch_scatter_delta(c);
}

// behind either solve: linear error of the step, the trial point, its error (gated by the linear cost change); the scalars on the host
static void evaluate_trial(gtg_context& c, FirstCallClock* first) {
  { PhaseTimer t(c, GTG_PH_LINEAR_ERROR); launch_linear_error(c); launch_smart_lin1(c); }
  { PhaseTimer t(c, GTG_PH_RETRACT); launch_retract(c); }
  { PhaseTimer t(c, GTG_PH_ERROR); const double* gate = c.scalars.p + (smart_gate(c) ? 2 * SC_COUNT : 0);
    launch_smart_triangulate(c, c.trial.p, gate, false); launch_error(c, c.trial.p, SC_TRIAL_ERROR, gate); }
  if (first) first->lap("linear error, retract, error");
  read_scalars(c);
}

// out[4] = linear error at zero and at the step, error of the trial point (inf: the model does not like the step), step length
static int trial_result(const gtg_context& c, bool solver_ok, double out[4]) {
  const double dsq = c.h_scalars[SC_DELTA_SQ];
  if (c.h_scalars[SC_FAIL] != 0.0 || !std::isfinite(dsq) || !solver_ok) return GTG_INDETERMINATE;
  out[0] = c.h_scalars[SC_LIN0];
  out[1] = c.h_scalars[SC_LIN1];
  out[2] = (out[0] - out[1] >= 0) ? c.h_scalars[SC_TRIAL_ERROR] : std::numeric_limits<double>::infinity();
  out[3] = std::sqrt(dsq);
  return GTG_OK;
}

int gtg_linearize(gtg_handle c) {
  GTG_TRY
  if (!c || !c->uploaded) throw std::invalid_argument("gtg_linearize: no problem uploaded");
  DeviceGuard on_device(c->device);
  if (c->n_smart) check_hip(hipMemsetAsync(c->scalars.p + SC_UNSUPPORTED, 0, sizeof(double), c->stream), "memset");
  FirstCallClock first(g_first_linearize, c->stream);
  { PhaseTimer t(*c, GTG_PH_LINEARIZE); launch_smart_triangulate(*c, c->values.p, nullptr, true); launch_linearize(*c); }
  first.lap("linearize");
  { PhaseTimer t(*c, GTG_PH_ASSEMBLE); launch_assemble(*c);
    if (c->n_smart) {   // the cameras' Hessian diagonal is that of the Schur-complemented smart factors: needs their E blocks (undamped)
      launch_point_eliminate(*c, 1.0, 0, 1e-6, 1e32);
      launch_smart_hdiag(*c);
    } }
  first.lap("assemble");
  exchange(*c, c->hdiag_red.p, c->NP);   // damping needs the full diagonal on every shard
  if (c->n_smart) {   // (sharded: every shard must see what any shard met)
    if (c->n_shards > 1) exchange(*c, c->scalars.p + SC_UNSUPPORTED, 1);
    check_hip(hipMemcpyAsync(c->h_scalars + SC_UNSUPPORTED, c->scalars.p + SC_UNSUPPORTED, sizeof(double), hipMemcpyDeviceToHost, c->stream), "D2H");
  }
  check_hip(hipStreamSynchronize(c->stream), "sync");
  collect(*c, {GTG_PH_LINEARIZE, GTG_PH_ASSEMBLE});
  check_smart_supported(*c, "gtg_linearize");
  c->linearized = true;
  return GTG_OK;
  GTG_CATCH
}

int gtg_try_lambda(gtg_handle c, double lambda, int diag, double dmin, double dmax, double out[4]) {
  GTG_TRY
  if (!c || !c->uploaded || !c->linearized) throw std::invalid_argument("gtg_try_lambda: call gtg_linearize first");
  if (!(lambda > 0.0)) throw std::invalid_argument("gtg_try_lambda: lambda must be > 0");
  DeviceGuard on_device(c->device);
  // The factorisation's kernels wait for each other inside a launch (dataflow schedule: two persistent kernels; stream schedule: the
  // TRSM workgroups of a panel launch).  A dependency wait that runs into its bound raises SC_TIMEOUT and the kernels drain: a chain
  // kernel that was not placed, a device shared with another process, or -- seen with several handles on one device -- a flag that an
  // XCD's L2 kept serving with its old value although the flags are published twice (chol_dataflow.hip::st_flag).  The try is then
  // repeated: first with the SAME schedule (a stuck wait is a property of one pass, not of the problem, and the repeat returns the
  // same bits as an undisturbed try: the trajectory does not depend on whether a wait timed out), then, should that time out as
  // well, with the other schedule (stream / event launches of cholesky.hip: kernels that never wait for a kernel launched after
  // them; its plan is always built; with one chain it runs the same sums in the same order, with several chains the cross-part
  // updates are summed in another order: the same numbers to rounding).  The reduced system is assembled again each time, because
  // the factorisation works in place.
  // Sharded: the scalars are summed over the shards by read_scalars, so every shard sees the time-out of any shard and all repeat.
  // (GTG_CHOL=streams: there is no other schedule to fall back to -- one repeat, then the error)
  const int max_attempts = c->use_df ? 3 : 2;
  FirstCallClock first(g_first_try, c->stream);
  for (int attempt = 0; attempt < max_attempts; attempt++) {
    const bool df = c->use_df && attempt != 2;
    check_hip(hipMemsetAsync(c->scalars.p + SC_FAIL, 0, 3 * sizeof(double), c->stream), "memset");
    { PhaseTimer t(*c, GTG_PH_POINT_ELIM); launch_point_eliminate(*c, lambda, diag, dmin, dmax); }
    first.lap("point elimination");
    { PhaseTimer t(*c, GTG_PH_SCHUR); launch_build_reduced(*c, lambda, diag, dmin, dmax); }
    first.lap("reduced system");
    exchange_reduced_system(*c);
    std::unique_lock<std::mutex> one_at_a_time;
    if (df) one_at_a_time = std::unique_lock<std::mutex>(df_device_lock(c->device));
    { PhaseTimer t(*c, GTG_PH_CHOLESKY);
      if (df) launch_cholesky_df(*c, smat(*c), c->NP, c->df, c->Dinv.p, c->scalars.p + SC_FAIL, c->pivot_kind.p, c->tile_exp.p);
      else launch_cholesky(*c, smat(*c), c->NP, c->plan, c->Dinv.p, c->scalars.p + SC_FAIL, c->pivot_kind.p, c->tile_exp.p); }
    first.lap("factorisation");
    { PhaseTimer t(*c, GTG_PH_SOLVE);
      launch_backward_solve(*c, smat(*c), c->NP, c->plan, c->Dinv.p, c->xred.p, c->scalars.p + SC_FAIL);
      launch_back_substitute(*c);
      first.lap("solves");
      if (c->n_shards > 1 && one_at_a_time.owns_lock()) {   // sharded: the exchange below may wait for another handle of this
        check_hip(hipStreamSynchronize(c->stream), "sync");   // process (two shards on one device in the tests): the factorisation is
        one_at_a_time.unlock();                                // done, let the other one start before waiting for it
      }
      scatter_step(*c); }
    evaluate_trial(*c, &first);
    if (one_at_a_time.owns_lock()) one_at_a_time.unlock();
    if (attempt + 1 < max_attempts && c->h_scalars[SC_TIMEOUT] != 0.0) {
      report_wait_timeout(*c, df, attempt);
      c->df_fallbacks++;
      continue;
    }
    break;
  }
  collect(*c, {GTG_PH_POINT_ELIM, GTG_PH_SCHUR, GTG_PH_CHOLESKY, GTG_PH_SOLVE, GTG_PH_LINEAR_ERROR, GTG_PH_RETRACT, GTG_PH_ERROR});
  c->have_trial = true;
  check_smart_supported(*c, "gtg_try_lambda");
  if (c->h_scalars[SC_TIMEOUT] != 0.0) throw std::runtime_error("gtg_try_lambda: a dependency wait of the factorisation ran into its bound (GPU shared or preempted?); the step was not computed");
  return trial_result(*c, true, out);
  GTG_CATCH
}

// Same contract as gtg_try_lambda, the damped system solved by block-Jacobi PCG on the implicit Schur complement
// (NonlinearOptimizerParams::Iterative + PCGSolverParameters in the reference, NonlinearOptimizer.cpp:154-172).
int gtg_try_lambda_pcg(gtg_handle c, double lambda, int diag, double dmin, double dmax, const double cg[4], double out[4],
                       int32_t* iterations) {
  GTG_TRY
  if (!c || !c->uploaded || !c->linearized) throw std::invalid_argument("gtg_try_lambda_pcg: call gtg_linearize first");
  if (!(lambda > 0.0) || !cg) throw std::invalid_argument("gtg_try_lambda_pcg: lambda must be > 0, cg = {max, min, eps_rel, eps_abs}");
  if (c->f.form == ProjForm::Planar) throw std::invalid_argument("gtg_try_lambda_pcg: a planar graph (POINT2 landmarks) is not supported, use gtg_try_lambda");
  DeviceGuard on_device(c->device);
  check_hip(hipMemsetAsync(c->scalars.p + SC_FAIL, 0, 3 * sizeof(double), c->stream), "memset");
  { PhaseTimer t(*c, GTG_PH_POINT_ELIM); launch_point_eliminate(*c, lambda, diag, dmin, dmax); }
  double g0 = 0.0, g1 = 0.0;
  int its = 0;
  { PhaseTimer t(*c, GTG_PH_CHOLESKY);
    its = launch_pcg(*c, lambda, diag, dmin, dmax, (int)cg[0], (int)cg[1], cg[2], cg[3], &g0, &g1); }
  if (iterations) *iterations = its;
  { PhaseTimer t(*c, GTG_PH_SOLVE);
    launch_back_substitute(*c);
    scatter_step(*c); }
  evaluate_trial(*c, nullptr);
  collect(*c, {GTG_PH_POINT_ELIM, GTG_PH_CHOLESKY, GTG_PH_SOLVE, GTG_PH_LINEAR_ERROR, GTG_PH_RETRACT, GTG_PH_ERROR});
  c->have_trial = true;
  check_smart_supported(*c, "gtg_try_lambda_pcg");
  return trial_result(*c, std::isfinite(g1), out);
  GTG_CATCH
}

int gtg_accept(gtg_handle c) {
  GTG_TRY
  if (!c || !c->have_trial) throw std::invalid_argument("gtg_accept: no trial values (call gtg_try_lambda)");
  DeviceGuard on_device(c->device);
  std::swap(c->values, c->trial);
  c->linearized = false; c->have_trial = false;
  return GTG_OK;
  GTG_CATCH
}

// Replicated handles (one per GPU, each holding the whole graph -- the speculative lambda search of gtsam_amd/speculative.py): the
// device addresses of the packed values for a device-to-device exchange run by the caller on the handle's stream.
int gtg_values_device_ptr(gtg_handle c, int which, void** ptr, int64_t* n_doubles, void** stream) {
  GTG_TRY
  if (!c || !c->uploaded || !ptr || (which != 0 && which != 1)) throw std::invalid_argument("gtg_values_device_ptr: no problem uploaded / bad arguments");
  if (which == 1 && !c->have_trial) throw std::invalid_argument("gtg_values_device_ptr: no trial values (call gtg_try_lambda)");
  *ptr = which == 0 ? (void*)c->values.p : (void*)c->trial.p;
  if (n_doubles) *n_doubles = c->user_val_size;
  if (stream) *stream = (void*)c->stream;
  return GTG_OK;
  GTG_CATCH
}
int gtg_values_changed(gtg_handle c) {
  GTG_TRY
  if (!c || !c->uploaded) throw std::invalid_argument("gtg_values_changed: no problem uploaded");
  DeviceGuard on_device(c->device);
  check_hip(hipStreamSynchronize(c->stream), "sync");
  c->linearized = false; c->have_trial = false;
  return GTG_OK;
  GTG_CATCH
}

int gtg_get_gradient(gtg_handle c, double* g, int64_t n) {
  GTG_TRY
  if (!c || !c->linearized || n != c->user_dim_size) throw std::invalid_argument("gtg_get_gradient: linearize first / wrong size");
  DeviceGuard on_device(c->device);
  std::vector<double> gr(9 * (size_t)std::max(c->n_red_vars, 1)), gp(3 * (size_t)std::max(c->n_lm, 1));
  check_hip(hipMemcpy(gr.data(), c->gred0.p, sizeof(double) * gr.size(), hipMemcpyDeviceToHost), "D2H");
  check_hip(hipMemcpy(gp.data(), c->gp.p, sizeof(double) * gp.size(), hipMemcpyDeviceToHost), "D2H");
  for (int v = 0; v < c->n_user_vars; v++) {   // (the hidden landmarks of smart factors are not the caller's variables)
    double* d = g + c->h_dim_off[v];
    if (c->h_lm_index[v] >= 0) for (int k = 0; k < 3; k++) d[k] = gp[3 * c->h_lm_index[v] + k];
    else for (int k = 0; k < c->h_red_dim[c->h_red_index[v]]; k++) d[k] = gr[9 * c->h_red_index[v] + k];
  }
  return GTG_OK;
  GTG_CATCH
}

// -gradientAtZero() of the caller's linearised graph: gtg_get_gradient, where every smart factor contributes as the Hessian factor it
// is in the reference -- its landmark eliminated WITHOUT damping (SmartProjectionFactor.h:190-233): the camera blocks lose
// F^T E (E^T E)^-1 E^T b.  Host arithmetic on the stored records of the smart measurements, in observation order; a failed track has
// zero records and contributes nothing, a point at infinity has a 2 x 2 landmark block (third row and column zero).
int gtg_get_graph_gradient(gtg_handle c, double* g, int64_t n) {
  const int rc = gtg_get_gradient(c, g, n);
  if (rc != GTG_OK || !c->n_smart) return rc;
  GTG_TRY
  DeviceGuard on_device(c->device);
  const HostIndex& hi = host_index(c);
  const bool pose = c->smart_pose;
  const int rec = pose ? kProjRec : kSfmRec, dc = pose ? 6 : 9, a2 = 2 * dc, bo = a2 + 6;
  const int64_t n_obs = pose ? c->f.n_proj : c->f.n_sfm, first = c->smart_obs0;
  if (pose && proj_rows(c->f.form) != 2) throw std::logic_error("gtg_get_graph_gradient: smart measurements in a three-row range");
  if (n_obs <= first) return GTG_OK;     // (the tracks of this graph live on other shards)
  std::vector<double> J((size_t)rec * (n_obs - first)), V(9 * (size_t)std::max(c->n_lm, 1)), gp(3 * (size_t)std::max(c->n_lm, 1));
  check_hip(hipMemcpy(J.data(), (pose ? c->f.proj_J.p : c->f.sfm_J.p) + (int64_t)rec * first, sizeof(double) * J.size(), hipMemcpyDeviceToHost), "D2H");
  check_hip(hipMemcpy(V.data(), c->V.p, sizeof(double) * V.size(), hipMemcpyDeviceToHost), "D2H");
  check_hip(hipMemcpy(gp.data(), c->gp.p, sizeof(double) * gp.size(), hipMemcpyDeviceToHost), "D2H");
  const std::vector<int32_t>& cam = pose ? hi.proj_pose : hi.sfm_cam;
  const std::vector<int32_t>& pt = pose ? hi.proj_point : hi.sfm_point;
  // x_l = (E^T E)^-1 E^T b per hidden landmark: Cholesky of the 3 x 3 (or leading 2 x 2) block
  std::vector<double> x(3 * (size_t)std::max(c->n_lm, 1), 0.0);
  for (int64_t i = 0; i < c->n_smart; i++) {
    const int l = c->h_lm_index[c->n_user_vars + i];
    const double* A = V.data() + 9 * (size_t)l; const double* b = gp.data() + 3 * (size_t)l; double* xl = x.data() + 3 * (size_t)l;
    const int d = (A[8] == 0.0 && A[2] == 0.0 && A[5] == 0.0) ? 2 : 3;
    if (A[0] == 0.0) continue;            // a track without a point: zero records
    double L[9] = {0};
    bool ok = true;
    for (int r = 0; r < d && ok; r++)
      for (int k = 0; k <= r; k++) {
        double s = A[3 * r + k];
        for (int m = 0; m < k; m++) s -= L[3 * r + m] * L[3 * k + m];
        if (k == r) { if (!(s > 0.0)) { ok = false; break; } L[3 * r + r] = std::sqrt(s); } else L[3 * r + k] = s / L[3 * k + k];
      }
    if (!ok) throw std::runtime_error("gtg_get_graph_gradient: the landmark block of a smart factor is not positive definite");
    double y[3] = {0, 0, 0};
    for (int r = 0; r < d; r++) { double s = b[r]; for (int m = 0; m < r; m++) s -= L[3 * r + m] * y[m]; y[r] = s / L[3 * r + r]; }
    for (int r = d - 1; r >= 0; r--) { double s = y[r]; for (int m = r + 1; m < d; m++) s -= L[3 * m + r] * xl[m]; xl[r] = s / L[3 * r + r]; }
  }
  for (int64_t o = first; o < n_obs; o++) {
    const double* R = J.data() + (size_t)rec * (o - first);
    const double* xl = x.data() + 3 * (size_t)c->h_lm_index[pt[(size_t)o]];
    double* d = g + c->h_dim_off[cam[(size_t)o]];
    for (int r = 0; r < 2; r++) {
      const double e = R[a2 + 3 * r] * xl[0] + R[a2 + 3 * r + 1] * xl[1] + R[a2 + 3 * r + 2] * xl[2];   // row r of E x
      for (int k = 0; k < dc; k++) d[k] -= R[dc * r + k] * e;
    }
  }
  (void)bo;
  return GTG_OK;
  GTG_CATCH
}

int gtg_get_hessian_diagonal(gtg_handle c, double* out, int64_t n) {
  GTG_TRY
  if (!c || !c->linearized || n != c->user_dim_size) throw std::invalid_argument("gtg_get_hessian_diagonal: linearize first / wrong size");
  DeviceGuard on_device(c->device);
  std::vector<double> hd(c->NP), V(9 * (size_t)std::max(c->n_lm, 1));
  check_hip(hipMemcpy(hd.data(), c->hdiag_red.p, sizeof(double) * hd.size(), hipMemcpyDeviceToHost), "D2H");
  check_hip(hipMemcpy(V.data(), c->V.p, sizeof(double) * V.size(), hipMemcpyDeviceToHost), "D2H");
  for (int v = 0; v < c->n_user_vars; v++) {
    double* d = out + c->h_dim_off[v];
    if (c->h_lm_index[v] >= 0) for (int k = 0; k < 3; k++) d[k] = V[9 * c->h_lm_index[v] + 4 * k];
    else { const int r = c->h_red_index[v]; for (int k = 0; k < c->h_red_dim[r]; k++) d[k] = hd[c->h_red_off[r] + k]; }
  }
  return GTG_OK;
  GTG_CATCH
}

int gtg_get_jacobians(gtg_handle c, int type, double* out, int64_t n) {
  GTG_TRY
  if (!c || !c->linearized) throw std::invalid_argument("gtg_get_jacobians: linearize first");
  DeviceGuard on_device(c->device);
  const double* src; int64_t cnt;
  switch (type) {
    case GTG_FAC_GENERAL_SFM: src = c->f.sfm_J.p; cnt = (c->n_smart && !c->smart_pose ? c->smart_obs0 : c->f.n_sfm) * kSfmRec; break;   // (not the observations of smart factors)
    case GTG_FAC_PROJECTION: src = c->f.proj_J.p; cnt = (c->smart_pose ? c->smart_obs0 : c->f.n_mono) * kProjRec; break;   // (not the observations of pose-type smart factors)
    case GTG_FAC_BETWEEN_POSE3: src = c->f.between_J.p; cnt = c->f.n_between * kBetweenRec; break;
    case GTG_FAC_PRIOR: src = c->f.prior_J.p; cnt = c->f.n_user_prior * kPriorRec; break;   // (not the partial pose priors behind them)
    case GTG_FAC_POSE_PARTIAL: src = c->f.prior_J.p + (int64_t)kPriorRec * c->f.n_user_prior; cnt = (c->f.n_prior - c->f.n_user_prior) * kPriorRec; break;
    case GTG_FAC_STEREO: src = c->f.proj_J.p + (int64_t)kStereoRec * c->f.n_mono; cnt = (c->f.n_cam - c->f.n_mono) * kStereoRec; break;
    case GTG_FAC_SAM: src = c->f.proj_J.p + (int64_t)kStereoRec * c->f.n_cam; cnt = has_sam(c->f.form) ? (c->f.n_proj - c->f.n_cam) * kStereoRec : 0; break;
    case GTG_FAC_SAM2: src = c->f.proj_J.p; cnt = c->f.form == ProjForm::Planar ? c->f.n_proj * kPlanarRec : 0; break;   // (a planar range holds nothing else)
    default: throw std::invalid_argument("unknown factor type");
  }
  if (n != cnt) throw std::invalid_argument("gtg_get_jacobians: wrong output size");
  DevBuf<double> recomputed;
  if (type == GTG_FAC_GENERAL_SFM && c->fused_sfm && cnt) {   // debug path: these records are not stored (fused.h) -- recomputed at the current values
    recomputed.alloc((size_t)cnt);
    launch_sfm_records(*c, recomputed.p);
    check_hip(hipStreamSynchronize(c->stream), "sync");
    src = recomputed.p;
  }
  if (type == GTG_FAC_PROJECTION && proj_rows(c->f.form) == 3 && cnt) {
    // beside stereo factors the monocular records are stored with three rows, the third zero: give back the two-row records
    // [A1 2x6 | A2 2x3 | b 2] they hold
    std::vector<double> wide((size_t)c->f.n_mono * kStereoRec);
    check_hip(hipMemcpy(wide.data(), src, sizeof(double) * wide.size(), hipMemcpyDeviceToHost), "D2H");
    for (int64_t i = 0; i < c->f.n_mono; i++) {
      const double* w = &wide[(size_t)i * kStereoRec];
      double* o = out + i * kProjRec;
      for (int k = 0; k < 12; k++) o[k] = w[k];
      for (int k = 0; k < 6; k++) o[12 + k] = w[18 + k];
      o[18] = w[27]; o[19] = w[28];
    }
    return GTG_OK;
  }
  if (cnt) check_hip(hipMemcpy(out, src, sizeof(double) * cnt, hipMemcpyDeviceToHost), "D2H");
  return GTG_OK;
  GTG_CATCH
}

int gtg_get_reduced_matrix(gtg_handle c, double* S, int64_t n_elems) {
  GTG_TRY
  if (!c || !c->uploaded || n_elems != c->n_red * c->n_red) throw std::invalid_argument("gtg_get_reduced_matrix: wrong size");
  DeviceGuard on_device(c->device);
  // S carries alignment gaps (identity rows) between the nested-dissection parts: copy the square part and compact it
  const int64_t n = c->n_red, NP = c->NP;
  // (the stored tiles are brought over and scattered into a dense array on the host; tiles without a slot are zero)
  std::vector<double> full((size_t)NP * NP, 0.0);
  {
    std::vector<double> tiles(c->S.n);
    check_hip(hipMemcpy(tiles.data(), c->S.p, sizeof(double) * tiles.size(), hipMemcpyDeviceToHost), "D2H");
    const int nt = (int)(NP / kTile);
    for (int I = 0; I < nt; I++)
      for (int J = 0; J < nt; J++) {
        const int32_t q = c->plan.h_slot[(size_t)I * nt + J];
        if (q < 0) continue;
        for (int r = 0; r < kTile; r++)
          std::memcpy(&full[((size_t)I * kTile + r) * NP + (size_t)J * kTile], &tiles[(size_t)q * kTileDoubles + (size_t)r * kTile], sizeof(double) * kTile);
      }
  }
  std::vector<char> is_pad((size_t)NP, 0);
  for (int64_t i : c->h_pad_index) is_pad[(size_t)i] = 1;
  std::vector<int64_t> keep; keep.reserve((size_t)n);
  for (int64_t i = 0; i < NP; i++) if (!is_pad[(size_t)i]) keep.push_back(i);
  if ((int64_t)keep.size() != n) throw std::runtime_error("gtg_get_reduced_matrix: padding bookkeeping is inconsistent");
  for (int64_t i = 0; i < n; i++)
    for (int64_t j = 0; j < n; j++) S[i * n + j] = full[(size_t)keep[(size_t)i] * NP + keep[(size_t)j]];
  return GTG_OK;
  GTG_CATCH
}

int gtg_set_allreduce(gtg_handle c, gtg_allreduce_fn fn, void* user) {
  if (!c) return GTG_ERR_USAGE;
  c->allreduce = fn; c->allreduce_user = user;
  return GTG_OK;
}

int gtg_enable_timing(gtg_handle c, int on) { if (!c) return GTG_ERR_USAGE; c->timing = on != 0; return GTG_OK; }
int gtg_reset_timing(gtg_handle c) {
  if (!c) return GTG_ERR_USAGE;
  for (int i = 0; i < GTG_PH_COUNT; i++) { c->phase_ms[i] = 0; c->phase_calls[i] = 0; }
  return GTG_OK;
}
int gtg_get_phase_ms(gtg_handle c, double* ms, int64_t* calls, int n) {
  if (!c || n < GTG_PH_COUNT) return GTG_ERR_USAGE;
  for (int i = 0; i < GTG_PH_COUNT; i++) { ms[i] = c->phase_ms[i]; if (calls) calls[i] = c->phase_calls[i]; }
  return GTG_OK;
}
double gtg_cholesky_flops(gtg_handle c) { return c ? c->chol_flops : 0.0; }
double gtg_cholesky_flops_executed(gtg_handle c) { return !c ? 0.0 : (c->use_df && c->df.flops_executed > 0.0) ? c->df.flops_executed : c->chol_flops; }
double gtg_cholesky_flops_block_level(gtg_handle c) {
  if (!c) return 0.0;
  try { join_block_level(*c); } catch (...) { return 0.0; }
  return c->chol_flops_block;
}
int64_t gtg_structure_hash(gtg_handle c) { return c ? (int64_t)(c->structure_hash & 0x7FFFFFFFFFFFFFFFull) : -1; }
int gtg_smart_repeated_keys(gtg_handle c) { return c && c->uploaded ? (c->smart_repeats ? 1 : 0) : -1; }
int64_t gtg_smart_lost_workspace(gtg_handle c) { return c && c->uploaded ? (int64_t)c->smart_lost_rows.n : -1; }

// TriangulationResult of every smart factor as the last gtg_error / gtg_linearize left it (SmartProjectionFactor::point()): the status
// word of that call and the hidden landmark's value slot, which the triangulation kernel wrote (zeros for a track without a point)
int gtg_get_smart_triangulation(gtg_handle c, int32_t* status, double* points3, int64_t n_smart) {
  GTG_TRY
  if (!c || !c->uploaded || !status || !points3 || n_smart != c->n_smart) throw std::invalid_argument("gtg_get_smart_triangulation: wrong size or no problem uploaded");
  if (!n_smart) return GTG_OK;
  if (!c->smart_last_status) throw std::invalid_argument("gtg_get_smart_triangulation: call gtg_error or gtg_linearize first");
  DeviceGuard on_device(c->device);
  std::vector<int64_t> ptr((size_t)n_smart + 1);
  check_hip(hipMemcpyAsync(status, c->smart_last_status, sizeof(int32_t) * n_smart, hipMemcpyDeviceToHost, c->stream), "D2H");
  check_hip(hipMemcpyAsync(points3, c->values.p + c->user_val_size, sizeof(double) * 3 * n_smart, hipMemcpyDeviceToHost, c->stream), "D2H");
  check_hip(hipMemcpyAsync(ptr.data(), c->smart_ptr.p, sizeof(int64_t) * (n_smart + 1), hipMemcpyDeviceToHost, c->stream), "D2H");
  check_hip(hipStreamSynchronize(c->stream), "sync");
  for (int64_t i = 0; i < n_smart; i++)
    if (ptr[(size_t)i + 1] == ptr[(size_t)i]) { status[i] = -1; points3[3 * i] = points3[3 * i + 1] = points3[3 * i + 2] = 0.0; }   // a track of another shard
  return GTG_OK;
  GTG_CATCH
}
double gtg_linearize_bytes(gtg_handle c) { return c ? c->lin_bytes : 0.0; }

// debug only (not in the public header): ms per K=256 trailing update over an m x m tile grid, with ablations
double gtg_debug_syrk_ms(gtg_handle c, int m, int abl, int reps) {
  try {
    DeviceGuard on_device(c->device);
    const int nt = m + 2;      // every tile of an nt x nt grid gets a slot
    DevBuf<double> S; S.alloc((size_t)nt * nt * kTileDoubles);
    std::vector<int32_t> hs((size_t)(nt + 1) * nt, -1);
    for (int q = 0; q < nt * nt; q++) hs[(size_t)q] = q;
    DevBuf<int32_t> slot; slot.upload(hs.data(), hs.size(), c->stream);
    check_hip(hipMemset(S.p, 0, sizeof(double) * S.n), "memset");
    return debug_time_syrk(*c, SMat{S.p, slot.p, nt}, m, abl, reps);
  } catch (const std::exception& e) { g_last_error = e.what(); return -1.0; }
}

// debug only (not in the public header): cycle stamps of k_potrf128 stages on a 128x128 SPD matrix
int gtg_debug_potrf_stamps(gtg_handle c, double* A128, long long* out15) {
  GTG_TRY
  DevBuf<long long> dbg; dbg.alloc(16);
  check_hip(hipMemset(dbg.p, 0, 16 * sizeof(long long)), "memset");
  g_potrf_dbg_set(dbg.p);
  const int rc = gtg_dense_cholesky_host(c, A128, 128, nullptr);
  g_potrf_dbg_set(nullptr);
  check_hip(hipMemcpy(out15, dbg.p, 15 * sizeof(long long), hipMemcpyDeviceToHost), "D2H");
  return rc;
  GTG_CATCH
}

// tests: the tile schedule of the reduced-system Cholesky as the kernels read it (index lists only)
int gtg_debug_plan_sizes(gtg_handle c, int64_t sizes[8]) {
  GTG_TRY
  if (!c || !c->uploaded || !sizes) throw std::invalid_argument("gtg_debug_plan_sizes: no problem uploaded");
  (void)hipSetDevice(c->device);
  ensure_stream_lists(c->plan, c->stream);
  const CholPlan& pl = c->plan;
  sizes[0] = pl.nt; sizes[1] = (int64_t)pl.rows.n; sizes[2] = (int64_t)pl.pairs.n; sizes[3] = (int64_t)pl.bcols.n;
  sizes[4] = pl.n_stored; sizes[5] = pl.n_exch; sizes[6] = (int64_t)pl.s1_off.size(); sizes[7] = (int64_t)pl.part_parent.size();
  return GTG_OK;
  GTG_CATCH
}
int gtg_debug_plan_lists(gtg_handle c, int32_t* rows, int32_t* pairs, int32_t* bcols, int32_t* stored, int32_t* exch,
                         int64_t* per_tile, int64_t* per_pair, int32_t* pair_part, int32_t* part_parent) {
  GTG_TRY
  if (!c || !c->uploaded) throw std::invalid_argument("gtg_debug_plan_lists: no problem uploaded");
  DeviceGuard on_device(c->device);
  (void)hipSetDevice(c->device);
  ensure_stream_lists(c->plan, c->stream);
  const CholPlan& pl = c->plan;
  auto down = [&](int32_t* dst, const DevBuf<int32_t>& b, size_t n) { if (dst && n) check_hip(hipMemcpy(dst, b.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost), "D2H"); };
  down(rows, pl.rows, pl.rows.n); down(pairs, pl.pairs, pl.pairs.n); down(bcols, pl.bcols, pl.bcols.n);
  down(stored, pl.stored, 2 * (size_t)pl.n_stored); down(exch, pl.exch, 2 * (size_t)pl.n_exch);
  if (per_tile) for (int k = 0; k < pl.nt; k++) { per_tile[4 * k] = pl.trsm_off[k]; per_tile[4 * k + 1] = pl.trsm_cnt[k]; per_tile[4 * k + 2] = pl.bwd_off[k]; per_tile[4 * k + 3] = pl.bwd_cnt[k]; }
  if (per_pair) for (size_t p = 0; p < pl.s1_off.size(); p++) {
    int64_t* q = per_pair + 8 * p;
    q[0] = pl.s1_off[p]; q[1] = pl.s1_cnt[p]; q[2] = pl.nar_off[p]; q[3] = pl.nar_cnt[p]; q[4] = pl.rest_off[p]; q[5] = pl.rest_cnt[p];
    q[6] = pl.anc_off[p]; q[7] = pl.anc_cnt[p];
  }
  if (pair_part) for (size_t p = 0; p < pl.pair_part.size(); p++) pair_part[p] = pl.pair_part[p];
  if (part_parent) for (size_t x = 0; x < pl.part_parent.size(); x++) part_parent[x] = pl.part_parent[x];
  return GTG_OK;
  GTG_CATCH
}

int gtg_debug_df_plan(gtg_handle c, int64_t sizes[4], int32_t* tasks, int32_t* klist) {
  GTG_TRY
  if (!c || !c->uploaded || !sizes) throw std::invalid_argument("gtg_debug_df_plan: no problem uploaded");
  const DfPlan& df = c->df;
  sizes[0] = df.nt; sizes[1] = df.n_tasks; sizes[2] = (int64_t)df.h_klist.size(); sizes[3] = c->use_df ? 1 : 0;
  if (tasks) std::copy(df.h_tasks.begin(), df.h_tasks.end(), tasks);
  if (klist) std::copy(df.h_klist.begin(), df.h_klist.end(), klist);
  return GTG_OK;
  GTG_CATCH
}

int gtg_debug_df_device_tables(gtg_handle c, int64_t sizes[3], int32_t* tasks, int32_t* steps, int32_t* chain) {
  GTG_TRY
  if (!c || !c->uploaded || !sizes) throw std::invalid_argument("gtg_debug_df_device_tables: no problem uploaded");
  const DfPlan& df = c->df;
  sizes[0] = (int64_t)df.tasks.n; sizes[1] = (int64_t)df.klist.n; sizes[2] = (int64_t)df.has_sub.n;
  (void)hipSetDevice(c->device);
  if (tasks && df.tasks.n) check_hip(hipMemcpyAsync(tasks, df.tasks.p, sizeof(int32_t) * df.tasks.n, hipMemcpyDeviceToHost, c->stream), "D2H");
  if (steps && df.klist.n) check_hip(hipMemcpyAsync(steps, df.klist.p, sizeof(int32_t) * df.klist.n, hipMemcpyDeviceToHost, c->stream), "D2H");
  if (chain && df.has_sub.n) check_hip(hipMemcpyAsync(chain, df.has_sub.p, sizeof(int32_t) * df.has_sub.n, hipMemcpyDeviceToHost, c->stream), "D2H");
  check_hip(hipStreamSynchronize(c->stream), "sync");
  return GTG_OK;
  GTG_CATCH
}

int gtg_debug_df_chains(gtg_handle c, int64_t sizes[3], int32_t* chain_off, int32_t* chain_tiles, int32_t* seq) {
  GTG_TRY
  if (!c || !c->uploaded || !sizes) throw std::invalid_argument("gtg_debug_df_chains: no problem uploaded");
  const DfPlan& df = c->df;
  sizes[0] = df.n_chain; sizes[1] = (int64_t)df.h_chain_tiles.size(); sizes[2] = (int64_t)df.h_seq.size();
  if (chain_off) std::copy(df.h_chain_off.begin(), df.h_chain_off.end(), chain_off);
  if (chain_tiles) std::copy(df.h_chain_tiles.begin(), df.h_chain_tiles.end(), chain_tiles);
  if (seq) std::copy(df.h_seq.begin(), df.h_seq.end(), seq);
  return GTG_OK;
  GTG_CATCH
}

int gtg_debug_reduced_order(gtg_handle c, int32_t* var_of_position, int32_t n) {
  GTG_TRY
  if (!c || !c->uploaded || !var_of_position || n != c->n_red_vars) throw std::invalid_argument("gtg_debug_reduced_order: no problem uploaded or wrong size");
  for (int r = 0; r < c->n_red_vars; r++) var_of_position[c->h_red_pos[r]] = c->h_red_var[r];
  return GTG_OK;
  GTG_CATCH
}

int gtg_debug_df_trace(gtg_handle c, int64_t* out, int64_t n) {
  GTG_TRY
  if (!c || !c->uploaded || !out || !c->df.trace.p || n != (int64_t)c->df.trace.n) throw std::invalid_argument("gtg_debug_df_trace: no trace (GTG_DF_TRACE=1 at upload) or wrong size");
  DeviceGuard on_device(c->device);
  check_hip(hipMemcpy(out, c->df.trace.p, sizeof(long long) * n, hipMemcpyDeviceToHost), "D2H");
  return GTG_OK;
  GTG_CATCH
}

int gtg_debug_df_ctrl(gtg_handle c, int32_t out[16]) {
  GTG_TRY
  if (!c || !c->uploaded || !out || !c->df.ctrl.p) throw std::invalid_argument("gtg_debug_df_ctrl: no dataflow schedule");
  DeviceGuard on_device(c->device);
  check_hip(hipMemcpy(out, c->df.ctrl.p, sizeof(int32_t) * 16, hipMemcpyDeviceToHost), "D2H");
  out[15] = (int32_t)c->df_fallbacks;   // (host counter) lambda tries repeated with the stream schedule after a time-out
  return GTG_OK;
  GTG_CATCH
}

int gtg_debug_df_poll_stats(gtg_handle c, int64_t out[5]) {
  GTG_TRY
  if (!c || !c->uploaded || !out || !c->df.ctrl.p) throw std::invalid_argument("gtg_debug_df_poll_stats: no dataflow schedule");
  DeviceGuard on_device(c->device);
  int32_t w[32];
  check_hip(hipMemcpy(w, c->df.ctrl.p, sizeof w, hipMemcpyDeviceToHost), "D2H");
  out[0] = w[18]; out[1] = w[7]; out[2] = w[16]; out[3] = w[6]; out[4] = w[17];
  return GTG_OK;
  GTG_CATCH
}

int gtg_dense_cholesky_host(gtg_handle c, double* A, int32_t n, double* rhs) {
  GTG_TRY
  if (!c || !A || n < 1) throw std::invalid_argument("gtg_dense_cholesky_host: bad arguments");
  DeviceGuard on_device(c->device);
  const int NP = (n + kTile - 1) / kTile * kTile;
  const int nt = NP / kTile;
  std::unique_lock<std::mutex> one_at_a_time;      // (declared before the buffers: they are released while it is held, on a throw as well)
  CholPlan plan;
  build_chol_plan(plan, nt, nullptr, c->stream);   // dense: every lower tile + the rhs row has a slot
  DevBuf<double> S, Dinv, x, fail;
  DfPlan df;
  const bool use_df = dataflow_schedule_selected();
  if (use_df) { plan_dataflow(df, nt, nullptr); upload_df_plan(df, c->stream, plan.h_slot, plan.n_stored); }   // (before S: the plan may want scratch slots behind the tiles)
  S.alloc((size_t)(plan.n_stored + df.n_scratch) * kTileDoubles); Dinv.alloc((size_t)nt * kTile * kTile); x.alloc(2 * (size_t)NP); fail.alloc(2);
  check_hip(hipMemset(Dinv.p, 0, sizeof(double) * Dinv.n), "memset");
  if (!c->chol_epoch_dev.p) { c->chol_epoch_dev.alloc(1); check_hip(hipMemset(c->chol_epoch_dev.p, 0, sizeof(long long)), "memset"); }
  check_hip(hipMemsetAsync(fail.p, 0, 2 * sizeof(double), c->stream), "memset");
  // the matrix by tiles (host side): lower triangle of A, identity on the padding, rhs in row 0 of the rhs tiles
  std::vector<double> tiles((size_t)plan.n_stored * kTileDoubles, 0.0);
  const SMat hs{tiles.data(), plan.h_slot.data(), nt};
  for (int64_t i = 0; i < n; i++) for (int64_t j = 0; j <= i; j++) *hs.at(i, j) = A[i * n + j];
  for (int64_t i = 0; i < n; i++) for (int64_t j = i + 1; j < std::min<int64_t>(n, (i / kTile + 1) * kTile); j++) *hs.at(i, j) = A[i * n + j];   // (upper part of the diagonal tiles, as the dense copy had it)
  for (int64_t i = n; i < NP; i++) *hs.at(i, i) = 1.0;
  if (rhs) for (int64_t j = 0; j < n; j++) *hs.at(NP, j) = rhs[j];
  check_hip(hipMemcpyAsync(S.p, tiles.data(), sizeof(double) * tiles.size(), hipMemcpyHostToDevice, c->stream), "H2D");
  const SMat Sm{S.p, plan.slot.p, nt};
  // rank test: the matrix is ONE frontal block, as in choleskyPartial(ABC, nFrontal = n) (base/cholesky.cpp:144-157)
  std::vector<unsigned char> pk(NP, 0);
  pk[n - 1] = n >= 2 ? 1 : 2;
  DevBuf<unsigned char> dpk; dpk.upload(pk.data(), pk.size(), c->stream);
  DevBuf<double> dexp; dexp.alloc(NP / kTile + 1);
  if (use_df) one_at_a_time = std::unique_lock<std::mutex>(df_device_lock(c->device));
  if (use_df) launch_cholesky_df(*c, Sm, NP, df, Dinv.p, fail.p, dpk.p, dexp.p);
  else launch_cholesky(*c, Sm, NP, plan, Dinv.p, fail.p, dpk.p, dexp.p);
  if (rhs) launch_backward_solve(*c, Sm, NP, plan, Dinv.p, x.p, fail.p);
  double hf2[2] = {0, 0};
  check_hip(hipMemcpyAsync(hf2, fail.p, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream), "D2H");
  check_hip(hipMemcpyAsync(tiles.data(), S.p, sizeof(double) * tiles.size(), hipMemcpyDeviceToHost, c->stream), "D2H");
  if (rhs) check_hip(hipMemcpyAsync(rhs, x.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream), "D2H");
  check_hip(hipStreamSynchronize(c->stream), "sync");
  for (int64_t i = 0; i < n; i++)       // the factor: lower triangle (and what the diagonal tiles hold above it, as before)
    for (int64_t j = 0; j < std::min<int64_t>(n, (i / kTile + 1) * kTile); j++) A[i * n + j] = *hs.at(i, j);
  if (hf2[1] != 0.0) throw std::runtime_error("gtg_dense_cholesky_host: a dependency wait of the factorisation ran into its bound");
  return hf2[0] != 0.0 ? GTG_INDETERMINATE : GTG_OK;
  GTG_CATCH
}

int64_t gtg_release_cached_memory(void) { destroy_parked(); return (int64_t)release_kept(-1); }
int64_t gtg_cached_memory_bytes(void) { return (int64_t)kept_bytes(); }

}  // extern "C"
