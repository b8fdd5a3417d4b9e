// device_memory.hip -- what a handle holds on its device and how it is released: the DevBuf bodies and the process' cache of big
// blocks behind them, the parked stream / event sets, the device guard of the entry points, the handle's constructor and destructor.
#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <stdexcept>
#include <string>

#include "analysis.h"
#include "kernels.h"

namespace gt {

void check_hip(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// The big buffers of a handle (>= 16 MB: the E slots, the term lists, the stored tiles of the reduced system) are kept for the next
// handle of the process when one is released instead of going back to the driver, at most GTG_ALLOC_CACHE_MB per DEVICE (default
// 2048 = about one handle of the headline size, 0.7 % of the device's memory; 0 switches it off); a kept block serves a request of
// 80 - 100 % of its size on the same device.  On boxes where the driver clears device memory as it hands it out a fresh hipMalloc costs
// ~30 ms per GB -- 10.9 of the 33 ms of a warm set-up of the L1723 shape in round 4, when the default was 0 -- and programs construct
// optimizers one after the other (GncOptimizer: one per outer iteration; the reference's own timing programs).  History of the
// default: 8192 in round 3 (the reduced system was a dense 1.9 GB - 31 GB array then), 0 in round 4, 2048 since round 5.  When an
// allocation fails, every kept block of that device is released and the allocation is tried once more;
// gtg_release_cached_memory() releases them at any time.  Every such buffer is fully written by the kernels before it is read, so
// recycled contents are never observed (GTG_ALLOC_POISON=1 fills a recycled block with NaNs first: a debug mode the parity suite
// can be run under).
namespace {
struct KeptBlock { void* p; size_t bytes; int device; };
std::mutex g_kept_mu;
std::vector<KeptBlock> g_kept;
constexpr size_t kKeepMin = (size_t)16 << 20;
size_t keep_limit() {
  static const size_t lim = [] { const char* e = std::getenv("GTG_ALLOC_CACHE_MB"); return (size_t)(e ? std::max(0L, std::atol(e)) : 2048L) << 20; }();
  return lim;
}
size_t kept_bytes_on(int dev) { size_t b = 0; for (const auto& k : g_kept) if (k.device == dev) b += k.bytes; return b; }   // (g_kept_mu held)
void* take_kept(size_t bytes, size_t* got) {
  if (bytes < kKeepMin || keep_limit() == 0) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(g_kept_mu);
  int best = -1;
  for (int i = 0; i < (int)g_kept.size(); i++)
    if (g_kept[i].device == dev && g_kept[i].bytes >= bytes && g_kept[i].bytes - bytes <= g_kept[i].bytes / 5 &&
        (best < 0 || g_kept[i].bytes < g_kept[best].bytes)) best = i;
  if (best < 0) return nullptr;
  void* q = g_kept[best].p;
  *got = g_kept[best].bytes;
  g_kept.erase(g_kept.begin() + best);
  static const bool poison = std::getenv("GTG_ALLOC_POISON") != nullptr;
  if (poison) (void)hipMemset(q, 0xFF, *got);   // all-ones bytes = a NaN in every double, -1 in every index
  return q;
}
bool keep_block(void* q, size_t bytes) {        // (hipFree synchronises the device; a kept block must be idle as well)
  if (bytes < kKeepMin || keep_limit() == 0) return false;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  std::lock_guard<std::mutex> lk(g_kept_mu);
  if (kept_bytes_on(dev) + bytes > keep_limit()) return false;
  if (hipDeviceSynchronize() != hipSuccess) return false;
  g_kept.push_back(KeptBlock{q, bytes, dev});
  return true;
}
}  // namespace

size_t release_kept(int dev) {                  // dev < 0: every device
  std::lock_guard<std::mutex> lk(g_kept_mu);
  size_t freed = 0;
  for (size_t i = 0; i < g_kept.size();) {
    if (dev < 0 || g_kept[i].device == dev) {
      int cur = 0;
      const bool sw = hipGetDevice(&cur) == hipSuccess && cur != g_kept[i].device && hipSetDevice(g_kept[i].device) == hipSuccess;
      (void)hipFree(g_kept[i].p);
      if (sw) (void)hipSetDevice(cur);
      freed += g_kept[i].bytes;
      g_kept.erase(g_kept.begin() + (long)i);
    } else i++;
  }
  return freed;
}
size_t kept_bytes() { std::lock_guard<std::mutex> lk(g_kept_mu); size_t b = 0; for (const auto& k : g_kept) b += k.bytes; return b; }

template <class T> void DevBuf<T>::alloc(size_t count) {
  free();
  n = count;
  if (!count) return;
  if (void* q = take_kept(sizeof(T) * count, &cap)) { p = static_cast<T*>(q); return; }
  hipError_t e = hipMalloc(&p, sizeof(T) * count);
  if (e != hipSuccess) {   // out of memory with blocks kept aside: give them back to the driver and try once more
    (void)hipGetLastError();
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && release_kept(dev) > 0) e = hipMalloc(&p, sizeof(T) * count);
  }
  if (e != hipSuccess) { p = nullptr; n = 0; }
  check_hip(e, "hipMalloc");
  cap = sizeof(T) * count;
}
template <class T> void DevBuf<T>::upload(const T* host, size_t count, hipStream_t s) {
  if (count != n || (count && !p)) alloc(count);
  if (count) check_hip(hipMemcpyAsync(p, host, sizeof(T) * count, hipMemcpyHostToDevice, s), "H2D");
}
template <class T> void DevBuf<T>::free() {
  if (p && !keep_block(p, cap ? cap : sizeof(T) * n)) (void)hipFree(p);
  p = nullptr; n = 0; cap = 0;
}
template struct DevBuf<double>;
template struct DevBuf<int32_t>;
template struct DevBuf<int64_t>;
template struct DevBuf<long long>;
template struct DevBuf<unsigned char>;

// Every entry point runs on the handle's device and leaves the caller's current device as it found it (a torch or multi-GPU host
// keeps its own notion of "current device").
DeviceGuard::DeviceGuard(int dev) {
  if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  if (prev != dev) check_hip(hipSetDevice(dev), "hipSetDevice"); else prev = -1;
}
DeviceGuard::~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }

// A handle's stream and events outlive it: gtg_destroy parks them (idle) per device and the next gtg_create of the process takes them from
// there -- creating a stream and 18 events cost 1.7 ms of every construction of an optimizer (tools/cpp/cold_start_probe.cpp), a third of
// what the whole symbolic analysis of the L1723 shape takes now.  At most kParkedMax sets per device are kept; gtg_release_cached_memory()
// destroys them with the cached device memory.
static std::mutex g_parked_mu;
static std::vector<ParkedQueue> g_parked;
constexpr size_t kParkedMax = 4;
bool take_parked(gtg_context& c) {
  if (std::getenv("GTG_NO_PARKED_STREAMS")) return false;   // (A/B: every handle creates its own stream and events)
  std::lock_guard<std::mutex> lk(g_parked_mu);
  for (size_t i = 0; i < g_parked.size(); i++)
    if (g_parked[i].device == c.device) {
      c.stream = g_parked[i].stream; c.copy_stream = g_parked[i].copy_stream; c.phase_events = std::move(g_parked[i].events);
      g_parked.erase(g_parked.begin() + (long)i);
      return true;
    }
  return false;
}
bool park_queue(ParkedQueue& q) {   // (the caller has synchronised the streams)
  if (std::getenv("GTG_NO_PARKED_STREAMS")) return false;
  std::lock_guard<std::mutex> lk(g_parked_mu);
  size_t n = 0;
  for (const auto& k : g_parked) n += k.device == q.device;
  if (n >= kParkedMax) return false;
  g_parked.push_back(std::move(q));
  return true;
}
void destroy_parked() {
  std::lock_guard<std::mutex> lk(g_parked_mu);
  int cur = 0; (void)hipGetDevice(&cur);
  for (auto& q : g_parked) {
    (void)hipSetDevice(q.device);
    for (hipEvent_t e : q.events) if (e) (void)hipEventDestroy(e);
    if (q.stream) (void)hipStreamDestroy(q.stream);
    if (q.copy_stream) (void)hipStreamDestroy(q.copy_stream);
  }
  g_parked.clear();
  (void)hipSetDevice(cur);
}

}  // namespace gt

gtg_context::gtg_context() = default;
gtg_context::~gtg_context() {
  if (block_level_thread.joinable()) block_level_thread.join();   // (a failure of the count, block_level_err, goes with the handle)
}
