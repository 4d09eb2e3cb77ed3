// tfidf_dist.hip — node level: documents sharded over GPUs, one shard
// (tfidf_index) per GPU, collectives between the shards (include/tfidf.h,
// "Node level").  Replaces the reference's Leader.start fan-out + merge
// (Leader.java:39-92: POST /worker/process to every worker, :51-70; sum per
// name, :73-77; TreeMap order, :80-88) over Worker.searchIndex
// (Worker.java:222-241), with the workers as GPU shards and RCCL collectives
// over xGMI in place of HTTP.
//
//   transports : caller callbacks (host or device buffers), the built-in RCCL
//                communicator (librccl of the HIP runtime this library runs on,
//                loaded at first use), or an in-process host transport for
//                shards of one process that share a device (tests).
//   tfidf_dist_*: per-rank (SPMD) orchestration: GLOBAL statistics by term
//                ownership, top-k / all-hits / batch merges of device merge
//                keys, SHARD mode's name table and Leader-style merge.
//   tfidf_node_*: one process owning every GPU of a device list: a worker
//                thread per shard runs the same per-rank orchestration.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <rccl/rccl.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/tfidf.h"
#include "analysis.h"
#include "compound_plan.h"
#include "compound_tree_plan.h"
#include "mlt_plan.h"
#include "tfidf_common.h"
#include "tfidf_internal.h"

using namespace tfidf;

namespace {

int errf(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int errf(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return set_error(code, buf);
}

#define DHIP(expr)                                                                                  \
  do {                                                                                              \
    hipError_t _e = (expr);                                                                         \
    if (_e != hipSuccess)                                                                           \
      return errf(TFIDF_E_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

struct DevGuard {
  int prev = -1;
  explicit DevGuard(int dev) {
    hipGetDevice(&prev);
    if (prev != dev) hipSetDevice(dev);
  }
  ~DevGuard() {
    int cur = -1;
    hipGetDevice(&cur);
    if (prev >= 0 && cur != prev) hipSetDevice(prev);
  }
};

struct DBuf {                      // device scratch, grown on demand, on the current device
  void *p = nullptr;
  size_t bytes = 0;
  int dev = -1;
  hipError_t reserve(size_t n) {
    int cur = -1;
    hipGetDevice(&cur);
    if (n <= bytes && p && cur == dev) return hipSuccess;
    release();                     // too small, or allocated on another device
    n = std::max<size_t>(n, 64);
    hipError_t e = hipMalloc(&p, n);
    if (e == hipSuccess) { bytes = n; hipGetDevice(&dev); }
    return e;
  }
  void release() {
    if (p) { DevGuard g(dev); hipFree(p); }
    p = nullptr;
    bytes = 0;
  }
  template <class T> T *as() const { return static_cast<T *>(p); }
  ~DBuf() { release(); }
};

struct HBuf {                      // pinned host scratch
  void *p = nullptr;
  size_t bytes = 0;
  hipError_t reserve(size_t n) {
    if (n <= bytes && p) return hipSuccess;
    if (p) { hipHostFree(p); p = nullptr; bytes = 0; }
    n = std::max<size_t>(n, 64);
    hipError_t e = hipHostMalloc(&p, n, hipHostMallocDefault);
    if (e == hipSuccess) bytes = n;
    return e;
  }
  template <class T> T *as() const { return static_cast<T *>(p); }
  ~HBuf() { if (p) hipHostFree(p); }
};

// ---------------------------------------------------------------------------
// transports

struct Transport {
  virtual ~Transport() {}
  virtual int kind() const = 0;                 // TFIDF_TRANSPORT_*
  virtual bool device_memory() const = 0;       // buffers are device memory (else host)
  virtual int all_gather(const void *send, void *recv, uint64_t bytes, hipStream_t s) = 0;
  virtual int all_to_all_v(const void *send, const uint64_t *sb, const uint64_t *so, void *recv, const uint64_t *rb,
                           const uint64_t *ro, hipStream_t s) = 0;
};

struct CallbackTransport : Transport {
  tfidf_collectives c;
  explicit CallbackTransport(const tfidf_collectives &x) : c(x) {}
  int kind() const override { return TFIDF_TRANSPORT_CALLBACK; }
  bool device_memory() const override { return c.memory == TFIDF_COLL_DEVICE; }
  int all_gather(const void *send, void *recv, uint64_t bytes, hipStream_t s) override {
    const int rc = c.all_gather(c.ctx, send, recv, bytes, (void *)s);
    return rc ? errf(TFIDF_E_HIP, "all_gather callback failed (%d)", rc) : TFIDF_OK;
  }
  int all_to_all_v(const void *send, const uint64_t *sb, const uint64_t *so, void *recv, const uint64_t *rb,
                   const uint64_t *ro, hipStream_t s) override {
    const int rc = c.all_to_all_v(c.ctx, send, sb, so, recv, rb, ro, (void *)s);
    return rc ? errf(TFIDF_E_HIP, "all_to_all_v callback failed (%d)", rc) : TFIDF_OK;
  }
};

// RCCL entry points, resolved from the librccl that sits next to the HIP
// runtime this library is bound to (a process with PyTorch loaded first runs
// the library on torch's runtime, whose directory holds its own librccl; a
// second RCCL bound to another runtime would not understand our streams).
struct RcclApi {
  bool ok = false;
  std::string err, path;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
};

RcclApi &rccl() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    std::vector<std::string> cand;
    Dl_info info;
    if (dladdr(reinterpret_cast<void *>(static_cast<hipError_t (*)(hipStream_t)>(&hipStreamSynchronize)), &info) && info.dli_fname) {
      std::string dir(info.dli_fname);
      const size_t sl = dir.rfind('/');
      dir = sl == std::string::npos ? std::string(".") : dir.substr(0, sl);
      cand.push_back(dir + "/librccl.so.1");
      cand.push_back(dir + "/librccl.so");
    }
    cand.push_back("/opt/rocm/lib/librccl.so.1");
    void *h = nullptr;
    for (const std::string &c : cand) {
      h = dlopen(c.c_str(), RTLD_NOW | RTLD_LOCAL);
      if (h) { api.path = c; break; }
    }
    if (!h) { api.err = std::string("librccl not found next to the HIP runtime: ") + dlerror(); return; }
    bool all = true;
    auto sym = [&](auto &fp, const char *name) {
      fp = reinterpret_cast<std::remove_reference_t<decltype(fp)>>(dlsym(h, name));
      all &= fp != nullptr;
    };
    sym(api.GetUniqueId, "ncclGetUniqueId");
    sym(api.CommInitRank, "ncclCommInitRank");
    sym(api.CommInitAll, "ncclCommInitAll");
    sym(api.CommDestroy, "ncclCommDestroy");
    sym(api.AllGather, "ncclAllGather");
    sym(api.Send, "ncclSend");
    sym(api.Recv, "ncclRecv");
    sym(api.GroupStart, "ncclGroupStart");
    sym(api.GroupEnd, "ncclGroupEnd");
    sym(api.GetErrorString, "ncclGetErrorString");
    if (!all) { api.err = "librccl lacks an entry point (" + api.path + ")"; return; }
    api.ok = true;
  });
  return api;
}

#define NCCL_TRY(expr)                                                                              \
  do {                                                                                              \
    ncclResult_t _r = (expr);                                                                       \
    if (_r != ncclSuccess) return errf(TFIDF_E_HIP, "%s: %s", #expr, rccl().GetErrorString(_r));    \
  } while (0)

struct RcclTransport : Transport {
  ncclComm_t comm = nullptr;
  int world = 1;
  RcclTransport(ncclComm_t c, int w) : comm(c), world(w) {}
  ~RcclTransport() override {
    if (comm) rccl().CommDestroy(comm);
  }
  int kind() const override { return TFIDF_TRANSPORT_RCCL; }
  bool device_memory() const override { return true; }
  int all_gather(const void *send, void *recv, uint64_t bytes, hipStream_t s) override {
    NCCL_TRY(rccl().AllGather(send, recv, bytes, ncclUint8, comm, s));
    return TFIDF_OK;
  }
  int all_to_all_v(const void *send, const uint64_t *sb, const uint64_t *so, void *recv, const uint64_t *rb,
                   const uint64_t *ro, hipStream_t s) override {
    // point-to-point pairs in one group: every xGMI link carries its own pair
    NCCL_TRY(rccl().GroupStart());
    for (int r = 0; r < world; r++) {
      if (sb[r]) NCCL_TRY(rccl().Send(static_cast<const uint8_t *>(send) + so[r], sb[r], ncclUint8, r, comm, s));
      if (rb[r]) NCCL_TRY(rccl().Recv(static_cast<uint8_t *>(recv) + ro[r], rb[r], ncclUint8, r, comm, s));
    }
    NCCL_TRY(rccl().GroupEnd());
    return TFIDF_OK;
  }
};

// Shards of one process exchanging through host memory (tfidf_node with a
// repeated device, or TFIDF_NODE_INPROC): a generation barrier around each
// exchange; each rank copies what it receives from the senders' buffers.
struct InprocGroup {
  int world;
  std::mutex mu;
  std::condition_variable cv;
  uint64_t phase = 0;
  int arrived = 0;
  std::vector<const void *> sp;
  std::vector<const uint64_t *> sb, so;
  explicit InprocGroup(int w) : world(w), sp(w), sb(w), so(w) {}
  void barrier() {
    std::unique_lock<std::mutex> lk(mu);
    const uint64_t my = phase;
    if (++arrived == world) {
      arrived = 0;
      phase++;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return phase != my; });
    }
  }
};

struct InprocTransport : Transport {
  std::shared_ptr<InprocGroup> g;
  int rank;
  InprocTransport(std::shared_ptr<InprocGroup> grp, int r) : g(std::move(grp)), rank(r) {}
  int kind() const override { return TFIDF_TRANSPORT_INPROC; }
  bool device_memory() const override { return false; }
  int all_gather(const void *send, void *recv, uint64_t bytes, hipStream_t) override {
    g->sp[rank] = send;
    g->barrier();
    for (int r = 0; r < g->world; r++)
      if (bytes) memcpy(static_cast<uint8_t *>(recv) + (size_t)r * bytes, g->sp[r], bytes);
    g->barrier();                                   // senders' buffers are free again
    return TFIDF_OK;
  }
  int all_to_all_v(const void *send, const uint64_t *sb, const uint64_t *so, void *recv, const uint64_t *rb,
                   const uint64_t *ro, hipStream_t) override {
    g->sp[rank] = send;
    g->sb[rank] = sb;
    g->so[rank] = so;
    g->barrier();
    int bad = -1;
    for (int r = 0; r < g->world; r++) {
      const uint64_t n = g->sb[r][rank];
      if (n != rb[r]) bad = r;
      else if (n) memcpy(static_cast<uint8_t *>(recv) + ro[r], static_cast<const uint8_t *>(g->sp[r]) + g->so[r][rank], n);
    }
    g->barrier();
    return bad >= 0 ? errf(TFIDF_E_INVALID_ARG, "all_to_all_v: rank %d sends a different size than rank %d expects",
                           bad, rank)
                    : TFIDF_OK;
  }
};

}  // namespace

// ---------------------------------------------------------------------------
// communicator: a transport + this rank's scratch and last results

struct tfidf_comm {
  int rank = 0, world = 1;
  int device = -1;                  // the communicator's GPU (RCCL), -1: the caller's current device
  std::unique_ptr<Transport> t;
  // staging between the transport's memory and the other kind
  DBuf d_stage_in, d_stage_out;
  HBuf h_stage_in, h_stage_out;
  // orchestration scratch (device)
  DBuf d_rec, d_cnt, d_got, d_ans, d_back, d_nu, d_keys, d_all, d_out, d_srt_k, d_srt_v, d_seg, d_tmp;
  HBuf h_out;
  // SHARD mode name table (tfidf_dist_shard_commit): every rank's names,
  // sorted by String.compareTo, distinct; this rank's doc -> name id
  std::string names;
  std::vector<uint64_t> name_off{0};
  DBuf d_name_of_doc;
  uint64_t names_gen = ~0ull;       // index commit generation the name table was built for
  bool names_ready = false;
  uint64_t global_gen = ~0ull;      // index commit generation of the last GLOBAL exchange
  uint64_t last_failed = 0;         // SHARD search: ranks skipped by the last search (bit r)
  HBuf h_hdr;                       // status words ahead of a rank's keys (pinned)
  DBuf d_meta, d_M;                 // GLOBAL exchange: this rank's meta row / every rank's (device)
  HBuf h_meta, h_M;                 // their pinned host sides
  bool hdr_pending = false;         // an upload out of h_hdr may still be queued (a search that failed)
  // last search results (tfidf_dist_last_hits / _last_names)
  std::vector<uint64_t> last_doc;
  std::vector<float> last_score;
  std::vector<uint32_t> last_name;
  std::vector<double> last_sum;
  uint64_t last_name_bytes = 0;
  // last SHARD batch (tfidf_dist_last_names_batch): every query's names, concatenated
  std::vector<uint32_t> batch_name;
  std::vector<double> batch_sum;
  std::vector<uint64_t> batch_qoff{0};    // [n_q + 1] query i's entries in batch_name / batch_sum
  uint64_t batch_name_bytes = 0;
};

namespace {

// gather `bytes` per rank: src / dst are device buffers (dev) or host buffers
int coll_gather(tfidf_comm *c, hipStream_t s, const void *src, void *dst, uint64_t bytes, bool dev) {
  const uint64_t tot = bytes * (uint64_t)c->world;
  if (bytes == 0) return TFIDF_OK;                        // every rank knows: no call
  if (c->t->device_memory() == dev) {
    if (dev) return c->t->all_gather(src, dst, bytes, s);
    return c->t->all_gather(src, dst, bytes, nullptr);
  }
  if (dev) {                                              // device data over a host transport
    DHIP(c->h_stage_in.reserve(bytes));
    DHIP(c->h_stage_out.reserve(tot));
    DHIP(hipMemcpyAsync(c->h_stage_in.p, src, bytes, hipMemcpyDeviceToHost, s));
    DHIP(hipStreamSynchronize(s));
    if (int rc = c->t->all_gather(c->h_stage_in.p, c->h_stage_out.p, bytes, nullptr)) return rc;
    DHIP(hipMemcpyAsync(dst, c->h_stage_out.p, tot, hipMemcpyHostToDevice, s));
    return TFIDF_OK;
  }
  // host data over a device transport
  DHIP(c->d_stage_in.reserve(bytes));
  DHIP(c->d_stage_out.reserve(tot));
  DHIP(hipMemcpyAsync(c->d_stage_in.p, src, bytes, hipMemcpyHostToDevice, s));
  if (int rc = c->t->all_gather(c->d_stage_in.p, c->d_stage_out.p, bytes, s)) return rc;
  DHIP(hipMemcpyAsync(dst, c->d_stage_out.p, tot, hipMemcpyDeviceToHost, s));
  DHIP(hipStreamSynchronize(s));
  return TFIDF_OK;
}

int coll_a2av(tfidf_comm *c, hipStream_t s, const void *src, const uint64_t *sb, const uint64_t *so, void *dst,
              const uint64_t *rb, const uint64_t *ro, bool dev) {
  uint64_t send_tot = 0, recv_tot = 0;
  for (int r = 0; r < c->world; r++) {
    send_tot = std::max(send_tot, so[r] + sb[r]);
    recv_tot = std::max(recv_tot, ro[r] + rb[r]);
  }
  if (c->t->device_memory() == dev) return c->t->all_to_all_v(src, sb, so, dst, rb, ro, dev ? s : nullptr);
  if (dev) {
    DHIP(c->h_stage_in.reserve(send_tot));
    DHIP(c->h_stage_out.reserve(recv_tot));
    if (send_tot) DHIP(hipMemcpyAsync(c->h_stage_in.p, src, send_tot, hipMemcpyDeviceToHost, s));
    DHIP(hipStreamSynchronize(s));
    if (int rc = c->t->all_to_all_v(c->h_stage_in.p, sb, so, c->h_stage_out.p, rb, ro, nullptr)) return rc;
    if (recv_tot) DHIP(hipMemcpyAsync(dst, c->h_stage_out.p, recv_tot, hipMemcpyHostToDevice, s));
    return TFIDF_OK;
  }
  DHIP(c->d_stage_in.reserve(send_tot));
  DHIP(c->d_stage_out.reserve(recv_tot));
  if (send_tot) DHIP(hipMemcpyAsync(c->d_stage_in.p, src, send_tot, hipMemcpyHostToDevice, s));
  if (int rc = c->t->all_to_all_v(c->d_stage_in.p, sb, so, c->d_stage_out.p, rb, ro, s)) return rc;
  if (recv_tot) DHIP(hipMemcpyAsync(dst, c->d_stage_out.p, recv_tot, hipMemcpyDeviceToHost, s));
  DHIP(hipStreamSynchronize(s));
  return TFIDF_OK;
}

// host all-gather of one u64 row per rank -> rows[world][n]
int gather_rows(tfidf_comm *c, hipStream_t s, const std::vector<uint64_t> &mine, std::vector<uint64_t> *rows) {
  rows->assign((size_t)c->world * mine.size(), 0);
  return coll_gather(c, s, mine.data(), rows->data(), mine.size() * 8, false);
}

// ---------------------------------------------------------------------------
// device kernels of the merges

// One thread per candidate key: its rank among the keys of every list of its
// query = its index in its own list + the keys above it in the others (lists
// are sorted descending; keys are distinct: global doc ids differ), found by
// binary search.  Candidates ranked below k_out are written at their rank.
__global__ void __launch_bounds__(256) k_merge_lists(const uint64_t *keys, uint32_t n_lists, uint64_t rstride,
                                                     uint64_t qstride, uint64_t len, uint32_t n_q, uint64_t *out,
                                                     uint64_t k_out) {
  const uint64_t per_q = (uint64_t)n_lists * len;
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= per_q * n_q) return;
  const uint32_t q = (uint32_t)(t / per_q);
  const uint64_t rem = t - (uint64_t)q * per_q;
  const uint32_t r = (uint32_t)(rem / len);
  const uint64_t i = rem - (uint64_t)r * len;
  const uint64_t x = keys[(uint64_t)r * rstride + (uint64_t)q * qstride + i];
  if (x == 0 || i >= k_out) return;
  uint64_t rank = i;
  for (uint32_t o = 0; o < n_lists && rank < k_out; o++) {
    if (o == r) continue;
    const uint64_t *l = keys + (uint64_t)o * rstride + (uint64_t)q * qstride;
    uint64_t a = 0, z = len;                    // first index whose key is < x (keys above x: [0, a))
    while (a < z) {
      const uint64_t m = (a + z) >> 1;
      if (l[m] > x) a = m + 1; else z = m;
    }
    rank += a;
  }
  if (rank < k_out) out[(uint64_t)q * k_out + rank] = x;
}

// SHARD mode: (name id << 32 | score bits) records of every hit key (local doc ids)
__global__ void k_name_records(const uint64_t *keys, uint64_t n, const uint32_t *name_of_doc, uint64_t *rec) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = keys[i];
  const uint32_t doc = ~(uint32_t)k;
  rec[i] = ((uint64_t)name_of_doc[doc] << 32) | (k >> 32);
}

// gathered [world][maxn] records (rows padded) -> key (name id) / value (score bits) arrays in rank order
__global__ void k_split_records(const uint64_t *all, uint64_t maxn, const uint64_t *row_n, const uint64_t *row_base,
                                uint32_t world, uint32_t *kk, uint32_t *vv) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= maxn * world) return;
  const uint32_t r = (uint32_t)(t / maxn);
  const uint64_t i = t - (uint64_t)r * maxn;
  if (i >= row_n[r]) return;
  const uint64_t x = all[t];
  kk[row_base[r] + i] = (uint32_t)(x >> 32);
  vv[row_base[r] + i] = (uint32_t)x;
}

__global__ void k_seg_heads(const uint32_t *k, uint64_t n, uint32_t *head) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) head[i] = (i == 0 || k[i] != k[i - 1]) ? 1u : 0u;
}

// Per name, the scores ((double) of each float) summed in rank order
// (HashMap.merge with Double::sum in worker-response order, Leader.java:73-77):
// the stable sort kept that order inside each name's run.
__global__ void k_seg_sums(const uint32_t *k, const uint32_t *v, const uint32_t *pos, uint64_t n, uint32_t *out_name,
                           double *out_sum) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || (i > 0 && k[i] == k[i - 1])) return;
  double s = (double)__uint_as_float(v[i]);
  for (uint64_t j = i + 1; j < n && k[j] == k[i]; j++) s += (double)__uint_as_float(v[j]);
  out_name[pos[i]] = k[i];
  out_sum[pos[i]] = s;
}

// All-hits batches: k_merge_lists from a fixed stride to CSR segments.  The
// gathered keys are [world][maxn]; rank r's row holds its chunk's hits
// query-major, query q's run at roff[r][q] .. roff[r][q + 1] (roff: [world][nc +
// 1]), each run sorted descending.  One thread per candidate key: its query by
// binary search in its rank's offsets, its output rank = its index in its own
// run + the keys above it in every other rank's run of the same query (binary
// search; keys are distinct: the doc ranges were checked disjoint).  Written
// decoded at out_off[q] + rank: global doc id (u64) and score (f32).  A wave's
// lanes hold consecutive keys of one run, so their searches in another run
// converge on neighbouring lines.
__global__ void __launch_bounds__(256) k_merge_segments(const uint64_t *keys, uint64_t maxn, uint32_t world,
                                                        uint32_t nc, const uint64_t *roff, const uint64_t *out_off,
                                                        uint64_t *out_doc, float *out_score) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= maxn * world) return;
  const uint32_t r = (uint32_t)(t / maxn);
  const uint64_t i = t - (uint64_t)r * maxn;
  const uint64_t *mo = roff + (uint64_t)r * (nc + 1);
  if (i >= mo[nc]) return;                        // the row's padding
  uint32_t lo = 0, hi = nc - 1;                   // last q with mo[q] <= i: mo[q] <= i < mo[q + 1]
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (mo[mid] <= i) lo = mid; else hi = mid - 1;
  }
  const uint32_t q = lo;
  const uint64_t x = keys[t];
  uint64_t rank = i - mo[q];
  for (uint32_t o = 0; o < world; o++) {
    if (o == r) continue;
    const uint64_t *oo = roff + (uint64_t)o * (nc + 1);
    const uint64_t *l = keys + (uint64_t)o * maxn + oo[q];
    uint64_t a = 0, z = oo[q + 1] - oo[q];        // first index whose key is < x (keys above x: [0, a))
    while (a < z) {
      const uint64_t m = (a + z) >> 1;
      if (l[m] > x) a = m + 1; else z = m;
    }
    rank += a;
  }
  const uint64_t at = out_off[q] + rank;
  out_doc[at] = (uint64_t)(~(uint32_t)x);
  out_score[at] = __uint_as_float((uint32_t)(x >> 32));
}

// SHARD batches: gathered [world][maxn] (name id << 32 | score bits) records, rank
// r's row query-major (roff as in k_merge_segments) -> key (query in chunk << 32 |
// name id) / value (score bits) arrays in rank order
__global__ void k_split_records_q(const uint64_t *all, uint64_t maxn, uint32_t world, uint32_t nc,
                                  const uint64_t *roff, const uint64_t *row_base, uint64_t *kk, uint32_t *vv) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= maxn * world) return;
  const uint32_t r = (uint32_t)(t / maxn);
  const uint64_t i = t - (uint64_t)r * maxn;
  const uint64_t *mo = roff + (uint64_t)r * (nc + 1);
  if (i >= mo[nc]) return;
  uint32_t lo = 0, hi = nc - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (mo[mid] <= i) lo = mid; else hi = mid - 1;
  }
  const uint64_t x = all[t];
  kk[row_base[r] + i] = ((uint64_t)lo << 32) | (x >> 32);
  vv[row_base[r] + i] = (uint32_t)x;
}

__global__ void k_seg_heads64(const uint64_t *k, uint64_t n, uint32_t *head) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) head[i] = (i == 0 || k[i] != k[i - 1]) ? 1u : 0u;
}

// k_seg_sums on (query, name) keys: per query and name, the double sum in rank
// order; the distinct keys (for the per-query bounds) and their name ids
__global__ void k_seg_sums64(const uint64_t *k, const uint32_t *v, const uint32_t *pos, uint64_t n, uint64_t *out_key,
                             uint32_t *out_name, double *out_sum) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || (i > 0 && k[i] == k[i - 1])) return;
  double s = (double)__uint_as_float(v[i]);
  for (uint64_t j = i + 1; j < n && k[j] == k[i]; j++) s += (double)__uint_as_float(v[j]);
  out_key[pos[i]] = k[i];
  out_name[pos[i]] = (uint32_t)k[i];
  out_sum[pos[i]] = s;
}

// per-query counts from the sorted distinct keys: bounds[q] = the first entry
// whose query is >= q (q = 0 .. nc), so query q's names are [bounds[q], bounds[q + 1])
__global__ void k_query_bounds(const uint64_t *keys, uint64_t n, uint32_t nc, uint64_t *bounds) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q > nc) return;
  uint64_t a = 0, z = n;
  while (a < z) {
    const uint64_t m = (a + z) >> 1;
    if ((keys[m] >> 32) < q) a = m + 1; else z = m;
  }
  bounds[q] = a;
}

inline unsigned grid_of(uint64_t n, unsigned b = 256) { return (unsigned)((n + b - 1) / b); }

}  // namespace

hipError_t tfidf::launch_merge_lists(const uint64_t *keys, uint32_t n_lists, uint64_t rstride, uint64_t qstride,
                                     uint64_t len, uint32_t n_q, uint64_t *out, uint64_t k_out, hipStream_t s) {
  hipError_t e = hipMemsetAsync(out, 0, (size_t)n_q * k_out * 8, s);
  if (e != hipSuccess) return e;
  const uint64_t n = (uint64_t)n_q * n_lists * len;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_merge_lists, dim3(grid_of(n)), dim3(256), 0, s, keys, n_lists, rstride, qstride, len, n_q, out,
                     k_out);
  return hipGetLastError();
}

namespace {

void decode_keys(const uint64_t *k, uint64_t n, uint64_t *doc, float *score) {
  for (uint64_t i = 0; i < n; i++) {
    doc[i] = (~k[i]) & 0xFFFFFFFFull;
    const uint32_t b = (uint32_t)(k[i] >> 32);
    memcpy(&score[i], &b, 4);
  }
}

// the query status every rank computes alike (no collective when it fails)
int query_status(const uint8_t *q, uint64_t n) {
  QueryPlan plan;
  const int rc = parse_query(q, n, &plan);
  if (rc == kQBadUtf8) return errf(TFIDF_E_UNSUPPORTED_QUERY, "query is not valid UTF-8");
  if (rc == kQSyntax) return errf(TFIDF_E_QUERY_SYNTAX, "query does not parse (QueryParser ParseException / TooManyClauses)");
  return TFIDF_OK;
}

int check_comm(tfidf_index *ix, tfidf_comm *c) {
  if (!ix || !c) return errf(TFIDF_E_INVALID_ARG, "NULL index or communicator");
  return TFIDF_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// communicators

extern "C" int tfidf_comm_create(int32_t rank, int32_t world, const tfidf_collectives *coll, tfidf_comm **out) {
  if (!coll || !out || !coll->all_gather || !coll->all_to_all_v) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  if (world < 1 || rank < 0 || rank >= world) return errf(TFIDF_E_INVALID_ARG, "rank %d / world %d", rank, world);
  if (coll->memory != TFIDF_COLL_HOST && coll->memory != TFIDF_COLL_DEVICE)
    return errf(TFIDF_E_INVALID_ARG, "memory must be TFIDF_COLL_HOST or TFIDF_COLL_DEVICE");
  tfidf_comm *c = new tfidf_comm();
  c->rank = rank;
  c->world = world;
  c->t.reset(new CallbackTransport(*coll));
  *out = c;
  return TFIDF_OK;
}

extern "C" int tfidf_rccl_unique_id(uint8_t id[128]) {
  if (!id) return errf(TFIDF_E_INVALID_ARG, "NULL id");
  RcclApi &api = rccl();
  if (!api.ok) return errf(TFIDF_E_NO_DEVICE, "%s", api.err.c_str());
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  ncclUniqueId u;
  NCCL_TRY(api.GetUniqueId(&u));
  memcpy(id, &u, 128);
  return TFIDF_OK;
}

extern "C" int tfidf_comm_init_rccl(const uint8_t id[128], int32_t rank, int32_t world, int32_t device,
                                    tfidf_comm **out) {
  if (!id || !out) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  if (world < 1 || rank < 0 || rank >= world) return errf(TFIDF_E_INVALID_ARG, "rank %d / world %d", rank, world);
  RcclApi &api = rccl();
  if (!api.ok) return errf(TFIDF_E_NO_DEVICE, "%s", api.err.c_str());
  DevGuard g(device);
  ncclUniqueId u;
  memcpy(&u, id, 128);
  ncclComm_t comm = nullptr;
  NCCL_TRY(api.CommInitRank(&comm, world, u, rank));
  tfidf_comm *c = new tfidf_comm();
  c->rank = rank;
  c->world = world;
  c->device = device;
  c->t.reset(new RcclTransport(comm, world));
  *out = c;
  return TFIDF_OK;
}

extern "C" int tfidf_comm_create_inproc(int32_t world, tfidf_comm **comms) {
  if (!comms || world < 1 || world > 1024) return errf(TFIDF_E_INVALID_ARG, "NULL comms or world out of range");
  auto grp = std::make_shared<InprocGroup>(world);
  for (int32_t i = 0; i < world; i++) {
    tfidf_comm *c = new tfidf_comm();
    c->rank = i;
    c->world = world;
    c->t.reset(new InprocTransport(grp, i));
    comms[i] = c;
  }
  return TFIDF_OK;
}

extern "C" int tfidf_comm_destroy(tfidf_comm *c) {
  delete c;
  return TFIDF_OK;
}

extern "C" int tfidf_comm_info(const tfidf_comm *c, int32_t *rank, int32_t *world, int32_t *transport) {
  if (!c) return errf(TFIDF_E_INVALID_ARG, "NULL communicator");
  if (rank) *rank = c->rank;
  if (world) *world = c->world;
  if (transport) *transport = c->t->kind();
  return TFIDF_OK;
}

extern "C" int tfidf_comm_selftest(tfidf_comm *c) {
  if (!c) return errf(TFIDF_E_INVALID_ARG, "NULL communicator");
  const int ws = c->world, me = c->rank;
  int cur = 0;
  hipGetDevice(&cur);
  DevGuard g(c->device >= 0 ? c->device : cur);      // staging buffers on the communicator's GPU
  hipStream_t s = nullptr;                            // (the null stream of that device)
  // all-gather of (rank, world) rows
  std::vector<uint64_t> rows;
  if (int rc = gather_rows(c, s, {(uint64_t)me, (uint64_t)ws, 0xC0FFEEull}, &rows)) return rc;
  for (int r = 0; r < ws; r++)
    if (rows[3 * r] != (uint64_t)r || rows[3 * r + 1] != (uint64_t)ws || rows[3 * r + 2] != 0xC0FFEEull)
      return errf(TFIDF_E_HIP, "selftest: all_gather row %d wrong", r);
  // all-to-all-v: rank me sends (me + 1) * (r + 1) bytes of value (me * 16 + r) & 0xFF to rank r
  std::vector<uint64_t> sb(ws), so(ws), rb(ws), ro(ws);
  uint64_t st = 0, rt = 0;
  for (int r = 0; r < ws; r++) {
    sb[r] = (uint64_t)(me + 1) * (r + 1);
    so[r] = st;
    st += sb[r];
    rb[r] = (uint64_t)(r + 1) * (me + 1);
    ro[r] = rt;
    rt += rb[r];
  }
  std::vector<uint8_t> snd(st), rcv(rt, 0xEE);
  for (int r = 0; r < ws; r++) memset(snd.data() + so[r], (me * 16 + r) & 0xFF, sb[r]);
  if (int rc = coll_a2av(c, s, snd.data(), sb.data(), so.data(), rcv.data(), rb.data(), ro.data(), false)) return rc;
  for (int r = 0; r < ws; r++)
    for (uint64_t i = 0; i < rb[r]; i++)
      if (rcv[ro[r] + i] != (uint8_t)((r * 16 + me) & 0xFF))
        return errf(TFIDF_E_HIP, "selftest: all_to_all_v bytes from rank %d wrong", r);
  return TFIDF_OK;
}

// ---------------------------------------------------------------------------
// process model (2): per-rank orchestration

// GLOBAL statistics by term ownership.  Meta row per rank: [records per owner
// (world) | docCount | sumTTF | seed attempt | error] — one host read; the
// ranks see each other's errors and seed attempts in it, so they fail, or
// re-commit under one seed, together.  Round 6: one host synchronisation per
// exchange (the gathered meta rows): the owner counts stay on the device
// (written by the partition straight into the meta row), the partition,
// reduction and df import queue without waiting, and the new statistics view
// is published behind an event the first search waits for.
extern "C" int tfidf_dist_global_commit(tfidf_index *ix, tfidf_comm *c, uint64_t *n_vocab, uint64_t *doc_count,
                                        uint64_t *sum_ttf) {
  if (int rc = check_comm(ix, c)) return rc;
  const int ws = c->world, me = c->rank;
  const size_t W = ws + 4;
  DevGuard g(index_device(ix));
  hipStream_t s = index_stream(ix);
  int local_err = index_committed(ix) ? TFIDF_OK : errf(TFIDF_E_STATE, "index not committed");
  std::string local_msg = local_err ? tfidf_last_error() : "";
  DHIP(c->d_meta.reserve(W * 8));
  DHIP(c->d_M.reserve((size_t)ws * W * 8));
  DHIP(c->h_meta.reserve(W * 8));
  DHIP(c->h_M.reserve((size_t)ws * W * 8));
  uint64_t *meta = c->h_meta.as<uint64_t>();
  const uint64_t *M = c->h_M.as<uint64_t>();
  uint64_t n_rec = 0;
  for (int round = 0;; round++) {
    tfidf_index_stats st{};
    if (!local_err) local_err = tfidf_stats(ix, &st);
    if (!local_err) {
      DHIP(c->d_rec.reserve(std::max<uint64_t>(st.num_terms, 1) * 24));
      local_err = vocab_partition_async(ix, (uint32_t)ws, c->d_rec.p, c->d_rec.bytes / 24, c->d_meta.p, &n_rec);
    }
    if (local_err && local_msg.empty()) local_msg = tfidf_last_error();
    if (local_err) DHIP(hipMemsetAsync(c->d_meta.p, 0, (size_t)ws * 8, s));
    meta[ws] = st.doc_count;
    meta[ws + 1] = st.sum_ttf;
    meta[ws + 2] = st.hash_rebuilds;
    meta[ws + 3] = local_err ? (uint64_t)local_err : 0;
    DHIP(hipMemcpyAsync(c->d_meta.as<uint64_t>() + ws, meta + ws, 4 * 8, hipMemcpyHostToDevice, s));
    if (int rc = coll_gather(c, s, c->d_meta.p, c->d_M.p, W * 8, true)) return rc;
    DHIP(hipMemcpyAsync(c->h_M.p, c->d_M.p, (size_t)ws * W * 8, hipMemcpyDeviceToHost, s));
    DHIP(hipStreamSynchronize(s));                    // the one host read (meta rows; h_meta reusable)
    for (int r = 0; r < ws; r++)
      if (M[r * W + ws + 3]) {
        if (r == me) return set_error(local_err, local_msg.c_str());
        return errf((int)M[r * W + ws + 3], "rank %d failed in the GLOBAL statistics exchange", r);
      }
    uint64_t top = 0;
    bool same = true;
    for (int r = 0; r < ws; r++) top = std::max(top, M[r * W + ws + 2]);
    for (int r = 0; r < ws; r++) same &= M[r * W + ws + 2] == top;
    if (same) break;
    if (round > 8) return errf(TFIDF_E_STATE, "hash seed agreement did not converge");
    // a shard met a hash collision and rebuilt under a later seed: keys are
    // matched across shards, so the shards below it re-commit under that
    // seed (which may collide there in turn: agree again next round)
    if (st.hash_rebuilds < top) {
      local_err = tfidf_set_hash_attempt(ix, (uint32_t)top);
      if (!local_err) local_err = tfidf_commit(ix);
      tfidf_set_hash_attempt(ix, 0);
      if (local_err) local_msg = tfidf_last_error();
    }
  }
  std::vector<uint64_t> sb(ws), so(ws), rb(ws), ro(ws), sb2(ws), so2(ws), rb2(ws), ro2(ws);
  uint64_t gdc = 0, gttf = 0, n_got = 0, at = 0, at2 = 0;
  for (int r = 0; r < ws; r++) {
    gdc += M[r * W + ws];
    gttf += M[r * W + ws + 1];
    sb[r] = M[me * W + r] * 24;
    so[r] = at;
    at += sb[r];
    rb[r] = M[r * W + me] * 24;
    ro[r] = n_got * 24;
    n_got += M[r * W + me];
    // answers travel back: one u32 per record
    sb2[r] = M[r * W + me] * 4;
    so2[r] = ro[r] / 6;
    rb2[r] = M[me * W + r] * 4;
    ro2[r] = at2;
    at2 += rb2[r];
  }
  DHIP(c->d_got.reserve(std::max<uint64_t>(n_got, 1) * 24));
  if (int rc = coll_a2av(c, s, c->d_rec.p, sb.data(), so.data(), c->d_got.p, rb.data(), ro.data(), true)) return rc;
  DHIP(c->d_ans.reserve(std::max<uint64_t>(n_got, 1) * 4));
  DHIP(c->d_nu.reserve(8));
  if (int rc = vocab_reduce_async(ix, c->d_got.p, n_got, c->d_ans.p, c->d_nu.p)) return rc;
  DHIP(c->d_back.reserve(std::max<uint64_t>(n_rec, 1) * 4));
  if (int rc = coll_a2av(c, s, c->d_ans.p, sb2.data(), so2.data(), c->d_back.p, rb2.data(), ro2.data(), true)) return rc;
  // the generation the view was published on (not re-read: a commit on another
  // thread may have landed since)
  uint64_t gen = 0;
  if (int rc = set_global_df_async(ix, c->d_back.p, n_rec, gdc, gttf, &gen)) return rc;
  c->global_gen = gen;
  if (n_vocab) {
    uint64_t nu = 0;
    DHIP(hipMemcpyAsync(&nu, c->d_nu.p, 8, hipMemcpyDeviceToHost, s));
    DHIP(hipStreamSynchronize(s));
    std::vector<uint64_t> rows;
    if (int rc = gather_rows(c, s, {nu}, &rows)) return rc;
    uint64_t tot = 0;
    for (uint64_t x : rows) tot += x;
    *n_vocab = tot;
  }
  if (doc_count) *doc_count = gdc;
  if (sum_ttf) *sum_ttf = gttf;
  return TFIDF_OK;
}

namespace {

// ---- search-time agreement (round-4 advisor finding).  Every rank's local
// status travels in the first collective of a search — as a header ahead of
// its top-k keys, or in the count row of a variable-length gather — so a rank
// that cannot serve (index not committed, re-committed since the last GLOBAL
// exchange or name table, doc range past 2^32, a failed local search) never
// leaves the others waiting in the data collective: GLOBAL searches then fail
// on every rank together; SHARD searches merge the healthy ranks' hits
// (Leader.start skips a failed worker, Leader.java:67-69).  The header also
// carries (doc_base, n_docs): GLOBAL merge keys must not collide, so
// overlapping doc ranges fail on every rank (TFIDF_E_INVALID_ARG).
constexpr uint64_t kHdr = 4;        // status words per rank: {rc, doc_base, n_docs, 0}

// One snapshot for a whole node-level search: the status check,
// the local search and the document count all read the reader it pins, so a
// commit landing on another thread meanwhile cannot mix generations.
struct Pinned {
  tfidf_reader *rd = nullptr;
  uint64_t gen = 0, nd = 0;
  Pinned() = default;
  Pinned(const Pinned &) = delete;
  Pinned &operator=(const Pinned &) = delete;
  ~Pinned() { if (rd) tfidf_reader_close(rd); }
  int open(tfidf_index *ix) {
    if (tfidf_reader_open(ix, &rd) != TFIDF_OK) { rd = nullptr; return errf(TFIDF_E_STATE, "index not committed"); }
    return tfidf_reader_info(rd, &gen, &nd);
  }
};

int local_search_status(Pinned &pin, tfidf_index *ix, tfidf_comm *c, uint64_t doc_base, bool global) {
  if (int rc = pin.open(ix)) return rc;
  if (doc_base + pin.nd > (1ull << 32))
    return errf(TFIDF_E_CAPACITY, "global doc ids must stay below 2^32 (merge keys carry 32-bit ids)");
  if (global && c->global_gen != pin.gen)
    return errf(TFIDF_E_STATE, "tfidf_dist_global_commit first (after every commit)");
  if (!global && (!c->names_ready || c->names_gen != pin.gen))
    return errf(TFIDF_E_STATE, "tfidf_dist_shard_commit first (after every commit)");
  return TFIDF_OK;
}

// Verdict over every rank's status words (rows of `stride` u64: rc, base, n):
// the first failing rank's error (its own message on that rank); GLOBAL mode
// also checks that the doc ranges do not overlap.  *failed = mask of failing ranks.
int status_verdict(tfidf_comm *c, const uint64_t *rows, size_t stride, int lrc, const std::string &lmsg,
                   bool fail_together, uint64_t *failed) {
  const int ws = c->world;
  uint64_t mask = 0;
  int first = -1;
  for (int r = 0; r < ws; r++)
    if (rows[(size_t)r * stride]) {
      if (r < 64) mask |= 1ull << r;
      if (first < 0) first = r;
    }
  if (failed) *failed = mask;
  if (first >= 0 && fail_together) {
    if (first == c->rank) return set_error(lrc, lmsg.c_str());
    return errf((int)rows[(size_t)first * stride], "rank %d cannot serve the search", first);
  }
  if (fail_together) {
    std::vector<std::pair<uint64_t, uint64_t>> rg;
    for (int r = 0; r < ws; r++)
      if (rows[(size_t)r * stride + 2]) rg.emplace_back(rows[(size_t)r * stride + 1], rows[(size_t)r * stride + 2]);
    std::sort(rg.begin(), rg.end());
    for (size_t i = 1; i < rg.size(); i++)
      if (rg[i - 1].first + rg[i - 1].second > rg[i].first)
        return errf(TFIDF_E_INVALID_ARG, "shard doc ranges overlap ([%llu, +%llu) and [%llu, +%llu))",
                    (unsigned long long)rg[i - 1].first, (unsigned long long)rg[i - 1].second,
                    (unsigned long long)rg[i].first, (unsigned long long)rg[i].second);
  }
  return TFIDF_OK;
}

int write_hits(tfidf_comm *c, uint64_t *doc_ids, float *scores, uint64_t cap, uint64_t *n_out) {
  const uint64_t n = c->last_doc.size();
  *n_out = n;
  const uint64_t m = std::min(n, cap);
  if (m && doc_ids) memcpy(doc_ids, c->last_doc.data(), m * 8);
  if (m && scores) memcpy(scores, c->last_score.data(), m * 4);
  if (n > cap) return errf(TFIDF_E_BUFFER, "%llu hits (tfidf_dist_last_hits holds them)", (unsigned long long)n);
  return TFIDF_OK;
}

// every hit's merge key of one query on this shard -> d_keys; *h = hits
int all_keys(Pinned &pin, tfidf_comm *c, const uint8_t *q, uint64_t q_len, uint64_t doc_base, uint64_t *h) {
  const uint64_t nd = std::max<uint64_t>(pin.nd, 1);
  DHIP(c->d_keys.reserve(nd * 8));
  return reader_all_keys_device(pin.rd, q, q_len, doc_base, c->d_keys.p, nd, h);
}

// gather variable-length device rows (d_keys[0, h)) from every rank, padded to
// the longest with `pad` -> d_all [world][maxn]; ns = every rank's count.  The
// count row carries the rank's status first (a failing rank sends h = 0).
int gather_var(tfidf_comm *c, hipStream_t s, uint64_t h, uint64_t pad_byte, int lrc, const std::string &lmsg,
               uint64_t doc_base, uint64_t n_docs, bool fail_together, std::vector<uint64_t> *ns, uint64_t *maxn) {
  if (lrc) h = 0;
  std::vector<uint64_t> rows;
  if (int rc = gather_rows(c, s, {(uint64_t)lrc, doc_base, n_docs, h}, &rows)) return rc;
  if (int rc = status_verdict(c, rows.data(), 4, lrc, lmsg, fail_together, &c->last_failed)) return rc;
  ns->assign(c->world, 0);
  uint64_t mx = 0;
  for (int r = 0; r < c->world; r++) {
    (*ns)[r] = rows[(size_t)r * 4 + 3];
    mx = std::max(mx, (*ns)[r]);
  }
  *maxn = mx;
  if (mx == 0) return TFIDF_OK;
  DHIP(c->d_out.reserve(mx * 8));
  if (h) DHIP(hipMemcpyAsync(c->d_out.p, c->d_keys.p, h * 8, hipMemcpyDeviceToDevice, s));
  if (mx > h) DHIP(hipMemsetAsync(c->d_out.as<uint64_t>() + h, (int)pad_byte, (mx - h) * 8, s));
  DHIP(c->d_all.reserve((size_t)c->world * mx * 8));
  return coll_gather(c, s, c->d_out.p, c->d_all.p, mx * 8, true);
}

// Top-k keys of this rank's n_q queries with the status header ahead of them
// (row = kHdr + n_q k words), all-gathered, merged per query on the device into
// d_out [n_q][k]; the merged keys and every rank's header are read back into
// h_out ([n_q k] keys, then [world][kHdr]).  A failing rank sends zero keys.
int gather_topk(tfidf_index *ix, tfidf_comm *c, hipStream_t s, uint64_t doc_base, const uint8_t *q_utf8,
                const uint64_t *q_offsets, uint32_t n_q, uint32_t k) {
  const int ws = c->world;
  const uint64_t per = (uint64_t)n_q * k, row = kHdr + per;
  DHIP(c->d_keys.reserve(row * 8));                    // only an allocation failure returns before the exchange
  DHIP(c->d_all.reserve((size_t)ws * row * 8));
  DHIP(c->d_out.reserve(per * 8));
  DHIP(c->h_out.reserve((per + (size_t)ws * kHdr) * 8));
  DHIP(c->h_hdr.reserve(kHdr * 8));
  uint64_t *dk = c->d_keys.as<uint64_t>();
  Pinned pin;
  int lrc = local_search_status(pin, ix, c, doc_base, true);
  if (!lrc) lrc = reader_batch_keys_device(pin.rd, q_utf8, q_offsets, n_q, k, doc_base, dk + kHdr);
  const std::string lmsg = lrc ? tfidf_last_error() : "";
  if (lrc) DHIP(hipMemsetAsync(dk + kHdr, 0, per * 8, s));
  uint64_t *hh = c->h_hdr.as<uint64_t>();
  if (c->hdr_pending) DHIP(hipStreamSynchronize(s));   // a failed search's header upload has left
  c->hdr_pending = true;
  hh[0] = (uint64_t)lrc;
  hh[1] = doc_base;
  hh[2] = lrc ? 0 : pin.nd;
  hh[3] = 0;
  DHIP(hipMemcpyAsync(dk, hh, kHdr * 8, hipMemcpyHostToDevice, s));
  if (int rc = coll_gather(c, s, dk, c->d_all.p, row * 8, true)) return rc;
  DHIP(launch_merge_lists(c->d_all.as<uint64_t>() + kHdr, (uint32_t)ws, row, k, k, n_q, c->d_out.as<uint64_t>(), k, s));
  uint64_t *ho = c->h_out.as<uint64_t>();
  DHIP(hipMemcpyAsync(ho, c->d_out.p, per * 8, hipMemcpyDeviceToHost, s));
  DHIP(hipMemcpy2DAsync(ho + per, kHdr * 8, c->d_all.p, row * 8, kHdr * 8, ws, hipMemcpyDeviceToHost, s));
  DHIP(hipStreamSynchronize(s));
  c->hdr_pending = false;
  return status_verdict(c, ho + per, kHdr, lrc, lmsg, true, nullptr);
}

}  // namespace

extern "C" int tfidf_dist_search(tfidf_index *ix, tfidf_comm *c, uint64_t doc_base, const uint8_t *q, uint64_t q_len,
                                 uint32_t k, uint64_t *doc_ids, float *scores, uint64_t cap, uint64_t *n_out) {
  if (int rc = check_comm(ix, c)) return rc;
  if (!n_out || (!q && q_len)) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  if (k > 1024) return errf(TFIDF_E_INVALID_ARG, "k must be <= 1024 (0 = all hits)");
  *n_out = 0;
  c->last_doc.clear();
  c->last_score.clear();
  if (int rc = query_status(q, q_len)) return rc;
  DevGuard g(index_device(ix));
  hipStream_t s = index_stream(ix);
  const int ws = c->world;
  uint64_t n = 0;
  if (k > 0) {
    const uint64_t offs[2] = {0, q_len};
    if (int rc = gather_topk(ix, c, s, doc_base, q, offs, 1, k)) return rc;
    const uint64_t *keys = c->h_out.as<uint64_t>();
    while (n < k && keys[n]) n++;
  } else {
    uint64_t h = 0, maxn = 0;
    Pinned pin;
    int lrc = local_search_status(pin, ix, c, doc_base, true);
    if (!lrc) lrc = all_keys(pin, c, q, q_len, doc_base, &h);
    const std::string lmsg = lrc ? tfidf_last_error() : "";
    std::vector<uint64_t> ns;
    if (int rc = gather_var(c, s, h, 0, lrc, lmsg, doc_base, lrc ? 0 : pin.nd, true, &ns, &maxn))
      return rc;
    for (uint64_t x : ns) n += x;
    if (n) {
      DHIP(c->d_tmp.reserve(n * 8));
      DHIP(launch_merge_lists(c->d_all.as<uint64_t>(), (uint32_t)ws, maxn, 0, maxn, 1, c->d_tmp.as<uint64_t>(), n, s));
      DHIP(c->h_out.reserve(n * 8));
      DHIP(hipMemcpyAsync(c->h_out.p, c->d_tmp.p, n * 8, hipMemcpyDeviceToHost, s));
      DHIP(hipStreamSynchronize(s));
    }
  }
  c->last_doc.resize(n);
  c->last_score.resize(n);
  decode_keys(c->h_out.as<uint64_t>(), n, c->last_doc.data(), c->last_score.data());
  return write_hits(c, doc_ids, scores, cap, n_out);
}

extern "C" int tfidf_dist_search_batch(tfidf_index *ix, tfidf_comm *c, uint64_t doc_base, const uint8_t *q_utf8,
                                       const uint64_t *q_offsets, uint32_t n_q, uint32_t k, uint64_t *doc_ids,
                                       float *scores, uint32_t *counts) {
  if (int rc = check_comm(ix, c)) return rc;
  if (!q_offsets || (n_q && (!doc_ids || !scores || !counts))) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  if (k == 0 || k > 1024) return errf(TFIDF_E_INVALID_ARG, "1 <= k <= 1024");
  if (n_q == 0) return TFIDF_OK;
  DevGuard g(index_device(ix));
  hipStream_t s = index_stream(ix);
  if (int rc = gather_topk(ix, c, s, doc_base, q_utf8, q_offsets, n_q, k)) return rc;
  const uint64_t *keys = c->h_out.as<uint64_t>();
  for (uint32_t i = 0; i < n_q; i++) {
    uint32_t m = 0;
    while (m < k && keys[(uint64_t)i * k + m]) m++;
    counts[i] = m;
    decode_keys(keys + (uint64_t)i * k, m, doc_ids + (uint64_t)i * k, scores + (uint64_t)i * k);
    for (uint32_t j = m; j < k; j++) {
      doc_ids[(uint64_t)i * k + j] = 0;
      scores[(uint64_t)i * k + j] = 0.0f;
    }
  }
  return TFIDF_OK;
}


namespace {
// SHARD search result with skipped ranks: TFIDF_OK (the healthy ranks' hits
// are the answer, as Leader.start returns the other workers' results), the
// skipped ranks in tfidf_dist_last_failed and, on every rank, a
// tfidf_last_error() message naming them (the failing rank's own reason there).
// When no rank could serve, every rank returns the (first) error instead.
int shard_partial(tfidf_comm *c, int lrc, const std::string &lmsg) {
  if (!c->last_failed) return TFIDF_OK;
  const int ws = std::min(c->world, 64);
  if (c->last_failed == (ws == 64 ? ~0ull : (1ull << ws) - 1)) {   // no rank answered: an error, not an empty map
    if (lrc) return set_error(lrc, lmsg.c_str());
    return errf(TFIDF_E_STATE, "no rank could serve the SHARD search");
  }
  std::string m = "SHARD search skipped rank(s)";
  for (int r = 0; r < c->world && r < 64; r++)
    if ((c->last_failed >> r) & 1u) m += " " + std::to_string(r);
  if (lrc) m += ": " + lmsg;
  set_error(lrc ? lrc : TFIDF_E_STATE, m.c_str());
  return TFIDF_OK;
}
}  // namespace

// SHARD mode name table: each rank sorts its own names (String.compareTo),
// the sorted lists are all-gathered and merged (distinct names in order);
// the rank's documents map to their name ids on the device.
extern "C" int tfidf_dist_shard_commit(tfidf_index *ix, tfidf_comm *c, uint64_t *n_names) {
  if (int rc = check_comm(ix, c)) return rc;
  const int ws = c->world, me = c->rank;
  DevGuard g(index_device(ix));
  hipStream_t s = index_stream(ix);
  c->names_ready = false;
  const uint64_t gen = index_generation(ix);
  int local_err = index_committed(ix) ? TFIDF_OK : errf(TFIDF_E_STATE, "index not committed");
  std::string local_msg = local_err ? tfidf_last_error() : "";
  const uint64_t nd = index_num_docs(ix);
  std::vector<uint64_t> offs(nd + 1, 0), perm(nd);
  std::string blob;
  if (!local_err) {
    uint64_t need = 0;
    int rc = tfidf_doc_keys(ix, nullptr, 0, offs.data(), &need);
    if (rc == TFIDF_OK || rc == TFIDF_E_BUFFER) {
      blob.resize(need);
      rc = tfidf_doc_keys(ix, reinterpret_cast<uint8_t *>(&blob[0]), need, offs.data(), &need);
    }
    if (!rc) rc = tfidf_sort_names(reinterpret_cast<const uint8_t *>(blob.data()), offs.data(), nd, perm.data());
    if (rc) { local_err = rc; local_msg = tfidf_last_error(); }
  }
  // sorted local names: lens + bytes
  std::vector<uint64_t> lens;
  std::string sorted;
  if (!local_err) {
    lens.resize(nd);
    sorted.reserve(blob.size());
    for (uint64_t i = 0; i < nd; i++) {
      const uint64_t d = perm[i];
      lens[i] = offs[d + 1] - offs[d];
      sorted.append(blob, offs[d], lens[i]);
    }
  }
  std::vector<uint64_t> M;
  if (int rc = gather_rows(c, s, {lens.size(), sorted.size(), (uint64_t)local_err}, &M)) return rc;
  for (int r = 0; r < ws; r++)
    if (M[3 * r + 2]) {
      if (r == me) return set_error(local_err, local_msg.c_str());
      return errf((int)M[3 * r + 2], "rank %d failed in the SHARD name exchange", r);
    }
  uint64_t maxn = 0, maxb = 0;
  for (int r = 0; r < ws; r++) { maxn = std::max(maxn, M[3 * r]); maxb = std::max(maxb, M[3 * r + 1]); }
  std::vector<uint64_t> all_lens((size_t)ws * maxn), mine_l(maxn, 0);
  std::vector<uint8_t> all_bytes((size_t)ws * maxb), mine_b(maxb, 0);
  std::copy(lens.begin(), lens.end(), mine_l.begin());
  std::copy(sorted.begin(), sorted.end(), mine_b.begin());
  if (int rc = coll_gather(c, s, mine_l.data(), all_lens.data(), maxn * 8, false)) return rc;
  if (int rc = coll_gather(c, s, mine_b.data(), all_bytes.data(), maxb, false)) return rc;
  // k-way merge of the sorted lists, distinct names
  struct Cur { uint64_t i = 0, pos = 0; };
  std::vector<Cur> cur(ws);
  c->names.clear();
  c->name_off.assign(1, 0);
  std::vector<uint32_t> my_nid(nd);
  auto name_of = [&](int r, const Cur &x, const uint8_t **p, uint64_t *n) {
    *p = all_bytes.data() + (size_t)r * maxb + x.pos;
    *n = all_lens[(size_t)r * maxn + x.i];
  };
  for (;;) {
    int best = -1;
    const uint8_t *bp = nullptr;
    uint64_t bn = 0;
    for (int r = 0; r < ws; r++) {
      if (cur[r].i >= M[3 * r]) continue;
      const uint8_t *p;
      uint64_t n;
      name_of(r, cur[r], &p, &n);
      if (best < 0 || utf16_compare(p, n, bp, bn) < 0) { best = r; bp = p; bn = n; }
    }
    if (best < 0) break;
    const uint32_t id = (uint32_t)(c->name_off.size() - 1);
    c->names.append(reinterpret_cast<const char *>(bp), bn);
    c->name_off.push_back(c->names.size());
    for (int r = 0; r < ws; r++) {                 // every list's copy of this name (byte-equal: same name)
      if (cur[r].i >= M[3 * r]) continue;
      const uint8_t *p;
      uint64_t n;
      name_of(r, cur[r], &p, &n);
      if (n == bn && memcmp(p, bp, n) == 0) {
        if (r == me) my_nid[perm[cur[r].i]] = id;
        cur[r].pos += n;
        cur[r].i++;
      }
    }
  }
  if (c->name_off.size() - 1 >= 0xFFFFFFFFull) return errf(TFIDF_E_CAPACITY, "more than 2^32 - 1 distinct names");
  DHIP(c->d_name_of_doc.reserve(std::max<uint64_t>(nd, 1) * 4));
  if (nd) DHIP(hipMemcpyAsync(c->d_name_of_doc.p, my_nid.data(), nd * 4, hipMemcpyHostToDevice, s));
  DHIP(hipStreamSynchronize(s));
  c->names_gen = gen;
  c->names_ready = true;
  if (n_names) *n_names = c->name_off.size() - 1;
  return TFIDF_OK;
}

extern "C" int tfidf_dist_shard_search(tfidf_index *ix, tfidf_comm *c, const uint8_t *q, uint64_t q_len,
                                       uint64_t *n_out, uint64_t *n_bytes) {
  if (int rc = check_comm(ix, c)) return rc;
  if (!n_out || (!q && q_len)) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  *n_out = 0;
  if (n_bytes) *n_bytes = 0;
  c->last_name.clear();
  c->last_sum.clear();
  c->last_name_bytes = 0;
  c->last_failed = 0;
  if (int rc = query_status(q, q_len)) return rc;
  DevGuard g(index_device(ix));
  hipStream_t s = index_stream(ix);
  const int ws = c->world;
  uint64_t h = 0, maxn = 0;
  // a rank that cannot serve (stale name table, failed local search) is a
  // failed worker: the others' hits are merged without it (Leader.java:67-69)
  Pinned pin;
  int lrc = local_search_status(pin, ix, c, 0, false);
  if (!lrc) lrc = all_keys(pin, c, q, q_len, 0, &h);            // local doc ids
  if (!lrc && h) {
    if (hipSuccess != c->d_tmp.reserve(h * 8)) lrc = errf(TFIDF_E_OOM, "name records: out of device memory");
    if (!lrc) {
      hipLaunchKernelGGL(k_name_records, dim3(grid_of(h)), dim3(256), 0, s, c->d_keys.as<uint64_t>(), h,
                         c->d_name_of_doc.as<uint32_t>(), c->d_tmp.as<uint64_t>());
      if (hipGetLastError() != hipSuccess ||
          hipMemcpyAsync(c->d_keys.p, c->d_tmp.p, h * 8, hipMemcpyDeviceToDevice, s) != hipSuccess)
        lrc = errf(TFIDF_E_HIP, "name records: launch failed");
    }
  }
  const std::string lmsg = lrc ? tfidf_last_error() : "";
  std::vector<uint64_t> ns;
  if (int rc = gather_var(c, s, h, 0, lrc, lmsg, 0, 0, false, &ns, &maxn)) return rc;
  uint64_t n = 0;
  std::vector<uint64_t> base(ws);
  for (int r = 0; r < ws; r++) { base[r] = n; n += ns[r]; }
  if (n == 0) return shard_partial(c, lrc, lmsg);
  if (n >= (1ull << 31)) return errf(TFIDF_E_CAPACITY, "too many hits to merge by name");
  // rank-order (name, score) pairs -> stable sort by name id -> per-name sums in rank order
  DHIP(c->d_srt_k.reserve(n * 16 + 2 * ws * 8));
  DHIP(c->d_srt_v.reserve(n * 16));
  uint32_t *k0 = c->d_srt_k.as<uint32_t>(), *k1 = k0 + n;
  uint64_t *rowinfo = reinterpret_cast<uint64_t *>(c->d_srt_k.as<uint8_t>() + n * 16);
  uint32_t *v0 = c->d_srt_v.as<uint32_t>(), *v1 = v0 + n;
  std::vector<uint64_t> info(2 * ws);
  for (int r = 0; r < ws; r++) { info[r] = ns[r]; info[ws + r] = base[r]; }
  DHIP(hipMemcpyAsync(rowinfo, info.data(), 2 * ws * 8, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_split_records, dim3(grid_of(maxn * ws)), dim3(256), 0, s, c->d_all.as<uint64_t>(), maxn, rowinfo,
                     rowinfo + ws, (uint32_t)ws, k0, v0);
  DHIP(hipGetLastError());
  size_t tmp_bytes = 0, t2 = 0;
  DHIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, k0, k1, v0, v1, (int)n, 0, 32, s));
  DHIP(c->d_seg.reserve(n * 12 + 16));
  uint32_t *head = c->d_seg.as<uint32_t>(), *pos = head + n, *out_name = pos + n;
  DHIP(hipcub::DeviceScan::ExclusiveSum(nullptr, t2, head, pos, (int)n, s));
  const size_t tcap = (std::max(tmp_bytes, t2) + 255) & ~(size_t)255;
  DHIP(c->d_tmp.reserve(tcap + n * 8));
  double *out_sum = reinterpret_cast<double *>(c->d_tmp.as<uint8_t>() + tcap);
  size_t tb = tcap;
  DHIP(hipcub::DeviceRadixSort::SortPairs(c->d_tmp.p, tb, k0, k1, v0, v1, (int)n, 0, 32, s));
  hipLaunchKernelGGL(k_seg_heads, dim3(grid_of(n)), dim3(256), 0, s, k1, n, head);
  tb = tcap;
  DHIP(hipcub::DeviceScan::ExclusiveSum(c->d_tmp.p, tb, head, pos, (int)n, s));
  hipLaunchKernelGGL(k_seg_sums, dim3(grid_of(n)), dim3(256), 0, s, k1, v1, pos, n, out_name, out_sum);
  DHIP(hipGetLastError());
  uint32_t last[2] = {0, 0};
  DHIP(hipMemcpyAsync(&last[0], pos + n - 1, 4, hipMemcpyDeviceToHost, s));
  DHIP(hipMemcpyAsync(&last[1], head + n - 1, 4, hipMemcpyDeviceToHost, s));
  DHIP(hipStreamSynchronize(s));
  const uint64_t nu = (uint64_t)last[0] + last[1];
  c->last_name.resize(nu);
  c->last_sum.resize(nu);
  DHIP(hipMemcpyAsync(c->last_name.data(), out_name, nu * 4, hipMemcpyDeviceToHost, s));
  DHIP(hipMemcpyAsync(c->last_sum.data(), out_sum, nu * 8, hipMemcpyDeviceToHost, s));
  DHIP(hipStreamSynchronize(s));
  uint64_t nb = 0;
  for (uint32_t id : c->last_name) nb += c->name_off[id + 1] - c->name_off[id];
  c->last_name_bytes = nb;
  *n_out = nu;
  if (n_bytes) *n_bytes = nb;
  return shard_partial(c, lrc, lmsg);
}

// ---------------------------------------------------------------------------
// all-hits batches (Worker.java:230 for a batch of requests, over the ranks)

namespace {

// Node chunks of an all-hits batch.  The first collective gathers every rank's
// per-query hit bound (the sum of the query's scoring terms' df, at most the
// shard's document count), so every rank derives the same chunk boundaries
// from the gathered bounds, `world` and this constant, never from a local
// value.  With B_r = rank r's bounds summed over the chunk's queries, a chunk
// takes queries while
//   world * max_r(B_r) * 8     the gathered buffer [world][longest row]
// + sum_r(B_r) * 12            the merged output (u64 doc + f32 score per hit;
//                              SHARD mode's sort buffers are charged the same)
// + max_r(B_r) * 8             the local key buffer (also the padded send row)
// stays within kDistAllHitsBudget, and while world * max_r(B_r) < 2^31 records.
// A chunk always holds at least one query.  1 GiB, as kAllHitsBudget bounds
// the local chunks inside it.  TFIDF_DIST_ALLHITS_CHUNK=<queries> fixes the
// chunk size (tests).
constexpr uint64_t kDistAllHitsBudget = 1ull << 30;

struct PreparedHolder {
  PreparedAllHits *p = nullptr;
  PreparedHolder() = default;
  PreparedHolder(const PreparedHolder &) = delete;
  PreparedHolder &operator=(const PreparedHolder &) = delete;
  ~PreparedHolder() { free_prepared_all_hits(p); }
};

struct BatchAll {
  tfidf_index *ix;
  tfidf_comm *c;
  hipStream_t s;
  uint32_t n_q;
  size_t stride;                      // words per rank in rows: kHdr + n_q
  Pinned pin;
  PreparedHolder pb;
  std::vector<uint64_t> rows;         // [world][kHdr + n_q]: every rank's status header and hit bounds
  int lrc = TFIDF_OK;                 // this rank's status at the first collective
  std::string lmsg;
  uint32_t fixed = 0;
  std::vector<uint64_t> B;            // [world] the current chunk's bounds per rank
  uint64_t maxB = 0, sumB = 0;

  // first collective: {rc, doc_base, n_docs, 0} + bounds; the verdict of every rank alike
  int first(uint64_t doc_base, bool global, const uint8_t *q_utf8, const uint64_t *q_offsets) {
    stride = kHdr + n_q;
    std::vector<uint64_t> mine(stride, 0);
    lrc = local_search_status(pin, ix, c, doc_base, global);
    if (!lrc) lrc = reader_prepare_all_hits(pin.rd, q_utf8, q_offsets, n_q, &pb.p, mine.data() + kHdr);
    lmsg = lrc ? tfidf_last_error() : "";
    if (lrc) std::fill(mine.begin() + kHdr, mine.end(), 0);      // a failing rank sends zeros
    mine[0] = (uint64_t)lrc;
    mine[1] = doc_base;
    mine[2] = lrc ? 0 : pin.nd;
    if (int rc = gather_rows(c, s, mine, &rows)) return rc;
    if (const char *e = knob("TFIDF_DIST_ALLHITS_CHUNK")) fixed = (uint32_t)std::max(1, atoi(e));
    B.assign(c->world, 0);
    return status_verdict(c, rows.data(), stride, lrc, lmsg, global, &c->last_failed);
  }

  // chunk [a, *z) from the gathered bounds (B, maxB, sumB: its per-rank bounds)
  int chunk(uint32_t a, uint32_t *z_out) {
    const int ws = c->world;
    std::fill(B.begin(), B.end(), 0);
    maxB = sumB = 0;
    uint32_t z = a;
    while (z < n_q) {
      uint64_t mx = 0, sum = 0;
      for (int r = 0; r < ws; r++) {
        const uint64_t b = B[r] + rows[(size_t)r * stride + kHdr + z];
        mx = std::max(mx, b);
        sum += b;
      }
      const bool records_ok = (uint64_t)ws * mx < (1ull << 31);
      if (z > a && (!records_ok || (fixed ? z - a >= fixed
                                          : (uint64_t)ws * mx * 8 + sum * 12 + mx * 8 > kDistAllHitsBudget)))
        break;
      if (!records_ok) return errf(TFIDF_E_CAPACITY, "query %u alone may have 2^31 hit records over the ranks", z);
      for (int r = 0; r < ws; r++) B[r] += rows[(size_t)r * stride + kHdr + z];
      maxB = mx;
      sumB = sum;
      z++;
    }
    *z_out = z;
    return TFIDF_OK;
  }

  // The chunk's count row: {rc} + this rank's per-query counts, gathered.  A
  // local failure since the first collective rides in it: every rank returns it
  // together here, before the data collective.  -> crow [world][1 + nc]
  int counts(uint32_t nc, int crc, const std::string &cmsg, const std::vector<uint64_t> &cnt,
             std::vector<uint64_t> *crow) {
    std::vector<uint64_t> mine(1 + (size_t)nc, 0);
    mine[0] = (uint64_t)crc;
    if (!crc) std::copy(cnt.begin(), cnt.begin() + nc, mine.begin() + 1);
    if (int rc = gather_rows(c, s, mine, crow)) return rc;
    for (int r = 0; r < c->world; r++)
      if ((*crow)[(size_t)r * (1 + nc)]) {
        if (r == c->rank) return set_error(crc, cmsg.c_str());
        return errf((int)(*crow)[(size_t)r * (1 + nc)], "rank %d failed inside the batch", r);
      }
    return TFIDF_OK;
  }
};

// offsets tables of a chunk from its count rows: roff [world][nc + 1] (each
// rank's per-query run starts within its row), per-rank totals, the longest row
void chunk_tables(const std::vector<uint64_t> &crow, int ws, uint32_t nc, std::vector<uint64_t> *roff,
                  std::vector<uint64_t> *row_n, uint64_t *maxn) {
  roff->assign((size_t)ws * (nc + 1), 0);
  row_n->assign(ws, 0);
  *maxn = 0;
  for (int r = 0; r < ws; r++) {
    uint64_t at = 0;
    for (uint32_t i = 0; i < nc; i++) {
      (*roff)[(size_t)r * (nc + 1) + i] = at;
      at += crow[(size_t)r * (1 + nc) + 1 + i];
    }
    (*roff)[(size_t)r * (nc + 1) + nc] = at;
    (*row_n)[r] = at;
    *maxn = std::max(*maxn, at);
  }
}

}  // namespace

extern "C" int tfidf_dist_search_batch_all(tfidf_index *ix, tfidf_comm *c, uint64_t doc_base, const uint8_t *q_utf8,
                                           const uint64_t *q_offsets, uint32_t n_q, uint64_t *doc_ids, float *scores,
                                           uint64_t cap, uint64_t *hit_offsets, uint64_t *n_out) {
  if (!ix || !c || !hit_offsets || !n_out || (n_q && !q_offsets) || (cap && (!doc_ids || !scores)))
    return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  for (uint32_t i = 0; i <= n_q; i++) hit_offsets[i] = 0;
  *n_out = 0;
  if (n_q == 0) return TFIDF_OK;                       // every rank knows: no collective
  DevGuard g(index_device(ix));
  BatchAll b{ix, c, index_stream(ix), n_q};
  hipStream_t s = b.s;
  const int ws = c->world;
  if (int rc = b.first(doc_base, true, q_utf8, q_offsets)) return rc;
  std::vector<uint64_t> cnt, crow, roff, row_n, tab;
  uint64_t total = 0;
  bool fits = true;
  for (uint32_t a = 0; a < n_q;) {
    uint32_t z = a;
    if (int rc = b.chunk(a, &z)) return rc;
    const uint32_t nc = z - a;
    // every allocation of the chunk, sized by the bounds, before the count row
    const bool deliver = cap > 0 && fits;
    int crc = TFIDF_OK;
    if (b.sumB) {
      bool ok = c->d_keys.reserve(b.maxB * 8) == hipSuccess && c->d_all.reserve((size_t)ws * b.maxB * 8) == hipSuccess;
      if (ok && deliver)
        ok = c->d_out.reserve(b.sumB * 8) == hipSuccess && c->d_tmp.reserve(b.sumB * 4) == hipSuccess &&
             c->d_seg.reserve(((size_t)ws + 1) * (nc + 1) * 8) == hipSuccess;
      if (!ok) crc = errf(TFIDF_E_OOM, "all-hits batch: out of device memory");
    }
    cnt.assign(nc, 0);
    uint64_t h = 0;
    if (!crc && b.sumB)
      crc = reader_batch_all_keys_device(b.pin.rd, b.pb.p, a, z, doc_base, c->d_keys.p, b.maxB, cnt.data(), &h);
    const std::string cmsg = crc ? tfidf_last_error() : "";
    if (int rc = b.counts(nc, crc, cmsg, cnt, &crow)) return rc;
    uint64_t maxn = 0;
    chunk_tables(crow, ws, nc, &roff, &row_n, &maxn);
    uint64_t H = 0;
    tab.assign(roff.begin(), roff.end());               // roff, then the chunk's output offsets
    for (uint32_t i = 0; i <= nc; i++) {
      tab.push_back(H);
      hit_offsets[a + i] = total + H;
      if (i < nc)
        for (int r = 0; r < ws; r++) H += crow[(size_t)r * (1 + nc) + 1 + i];
    }
    fits = fits && total + H <= cap;
    if (maxn) {
      // the key rows, padded to the longest rank's (like gather_var)
      if (maxn > h) DHIP(hipMemsetAsync(c->d_keys.as<uint64_t>() + h, 0, (maxn - h) * 8, s));
      if (int rc = coll_gather(c, s, c->d_keys.p, c->d_all.p, maxn * 8, true)) return rc;
      if (cap > 0 && fits) {
        uint64_t *d_tab = c->d_seg.as<uint64_t>();
        DHIP(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_merge_segments, dim3(grid_of(maxn * ws)), dim3(256), 0, s, c->d_all.as<uint64_t>(), maxn,
                           (uint32_t)ws, nc, d_tab, d_tab + (size_t)ws * (nc + 1), c->d_out.as<uint64_t>(),
                           c->d_tmp.as<float>());
        DHIP(hipGetLastError());
        // the chunk's (doc, score) arrays straight into the caller's, at the running offset
        DHIP(hipMemcpyAsync(doc_ids + total, c->d_out.p, H * 8, hipMemcpyDeviceToHost, s));
        DHIP(hipMemcpyAsync(scores + total, c->d_tmp.p, H * 4, hipMemcpyDeviceToHost, s));
      }
      DHIP(hipStreamSynchronize(s));                    // the chunk's buffers are free again
    }
    total += H;
    a = z;
  }
  hit_offsets[n_q] = total;
  *n_out = total;
  if (!fits) return errf(TFIDF_E_BUFFER, "need %llu result slots", (unsigned long long)total);
  return TFIDF_OK;
}

extern "C" int tfidf_dist_shard_search_batch(tfidf_index *ix, tfidf_comm *c, const uint8_t *q_utf8,
                                             const uint64_t *q_offsets, uint32_t n_q, uint64_t *n_out,
                                             uint64_t *n_bytes) {
  if (!ix || !c || !n_out || (n_q && !q_offsets)) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  *n_out = 0;
  if (n_bytes) *n_bytes = 0;
  c->batch_name.clear();
  c->batch_sum.clear();
  c->batch_qoff.assign((size_t)n_q + 1, 0);
  c->batch_name_bytes = 0;
  c->last_failed = 0;
  if (n_q == 0) return TFIDF_OK;
  DevGuard g(index_device(ix));
  BatchAll b{ix, c, index_stream(ix), n_q};
  hipStream_t s = b.s;
  const int ws = c->world;
  // a rank that cannot serve here is skipped for the whole batch (a failed
  // worker, Leader.java:67-69): it sends zero bounds, then zero counts
  // profiling only (TFIDF_HOST_TIMING): wall time of the call's stages on this rank
  using clk = std::chrono::steady_clock;
  const bool timing = knob("TFIDF_HOST_TIMING") != nullptr;
  double t_stage[5] = {0, 0, 0, 0, 0};          // first collective, local search, collectives, device merge, read-back
  clk::time_point t_at = clk::now();
  auto lap = [&](int stage) {
    if (!timing) return;
    const clk::time_point t = clk::now();
    t_stage[stage] += std::chrono::duration<double, std::milli>(t - t_at).count();
    t_at = t;
  };
  if (int rc = b.first(0, false, q_utf8, q_offsets)) return rc;
  lap(0);
  if (c->last_failed == (ws >= 64 ? ~0ull : (1ull << ws) - 1)) return shard_partial(c, b.lrc, b.lmsg);
  std::vector<uint64_t> cnt, crow, roff, row_n, tab, qb;
  for (uint32_t a = 0; a < n_q;) {
    uint32_t z = a;
    if (int rc = b.chunk(a, &z)) return rc;
    const uint32_t nc = z - a;
    uint32_t qbits = 1;
    while ((1ull << qbits) < nc) qbits++;
    const uint64_t N = b.sumB;                          // at most this many records in the chunk
    int crc = TFIDF_OK;
    size_t tcap = 0;
    if (N) {
      size_t t1 = 0, t2 = 0;
      hipcub::DeviceRadixSort::SortPairs(nullptr, t1, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                         (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)N, 0, (int)(32 + qbits), s);
      hipcub::DeviceScan::ExclusiveSum(nullptr, t2, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)N, s);
      tcap = (std::max(t1, t2) + 255) & ~(size_t)255;
      const bool ok = c->d_keys.reserve(b.maxB * 8) == hipSuccess && c->d_out.reserve(b.maxB * 8) == hipSuccess &&
                      c->d_all.reserve((size_t)ws * b.maxB * 8) == hipSuccess &&
                      c->d_srt_k.reserve(N * 16) == hipSuccess && c->d_srt_v.reserve(N * 8) == hipSuccess &&
                      c->d_seg.reserve(N * 20) == hipSuccess && c->d_tmp.reserve(tcap + N * 8) == hipSuccess &&
                      c->d_got.reserve((((size_t)ws + 2) * (nc + 1) + ws) * 8) == hipSuccess;
      if (!ok) crc = errf(TFIDF_E_OOM, "all-hits batch: out of device memory");
    }
    cnt.assign(nc, 0);
    uint64_t h = 0;
    if (!crc && !b.lrc && b.B[c->rank])
      crc = reader_batch_all_keys_device(b.pin.rd, b.pb.p, a, z, 0, c->d_keys.p, b.maxB, cnt.data(), &h);   // local ids
    if (!crc && h) {                                    // (name id << 32 | score bits) records -> the send row
      hipLaunchKernelGGL(k_name_records, dim3(grid_of(h)), dim3(256), 0, s, c->d_keys.as<uint64_t>(), h,
                         c->d_name_of_doc.as<uint32_t>(), c->d_out.as<uint64_t>());
      if (hipGetLastError() != hipSuccess) crc = errf(TFIDF_E_HIP, "name records: launch failed");
    }
    const std::string cmsg = crc ? tfidf_last_error() : "";
    lap(1);
    if (int rc = b.counts(nc, crc, cmsg, cnt, &crow)) return rc;
    uint64_t maxn = 0, n = 0;
    chunk_tables(crow, ws, nc, &roff, &row_n, &maxn);
    if (maxn) {
      if (maxn > h) DHIP(hipMemsetAsync(c->d_out.as<uint64_t>() + h, 0, (maxn - h) * 8, s));
      if (int rc = coll_gather(c, s, c->d_out.p, c->d_all.p, maxn * 8, true)) return rc;
      lap(2);
      tab.assign(roff.begin(), roff.end());             // roff, then every rank's first record in rank order
      for (int r = 0; r < ws; r++) { tab.push_back(n); n += row_n[r]; }
      uint64_t *d_tab = c->d_got.as<uint64_t>();
      DHIP(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
      // rank-order (query, name) / score pairs -> stable sort -> per (query, name) sums in rank order
      uint64_t *k0 = c->d_srt_k.as<uint64_t>(), *k1 = k0 + n;
      uint32_t *v0 = c->d_srt_v.as<uint32_t>(), *v1 = v0 + n;
      uint64_t *out_key = c->d_seg.as<uint64_t>();
      uint32_t *head = reinterpret_cast<uint32_t *>(out_key + n), *pos = head + n, *out_name = pos + n;
      double *out_sum = reinterpret_cast<double *>(c->d_tmp.as<uint8_t>() + tcap);
      uint64_t *d_qb = d_tab + tab.size();
      hipLaunchKernelGGL(k_split_records_q, dim3(grid_of(maxn * ws)), dim3(256), 0, s, c->d_all.as<uint64_t>(), maxn,
                         (uint32_t)ws, nc, d_tab, d_tab + (size_t)ws * (nc + 1), k0, v0);
      DHIP(hipGetLastError());
      size_t tb = 0;
      DHIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, k0, k1, v0, v1, (int)n, 0, (int)(32 + qbits), s));
      if (tb > tcap) return errf(TFIDF_E_HIP, "name sort: temporary storage beyond the chunk's reservation");
      tb = tcap;
      DHIP(hipcub::DeviceRadixSort::SortPairs(c->d_tmp.p, tb, k0, k1, v0, v1, (int)n, 0, (int)(32 + qbits), s));
      hipLaunchKernelGGL(k_seg_heads64, dim3(grid_of(n)), dim3(256), 0, s, k1, n, head);
      tb = tcap;
      DHIP(hipcub::DeviceScan::ExclusiveSum(c->d_tmp.p, tb, head, pos, (int)n, s));
      hipLaunchKernelGGL(k_seg_sums64, dim3(grid_of(n)), dim3(256), 0, s, k1, v1, pos, n, out_key, out_name, out_sum);
      DHIP(hipGetLastError());
      uint32_t last[2] = {0, 0};
      DHIP(hipMemcpyAsync(&last[0], pos + n - 1, 4, hipMemcpyDeviceToHost, s));
      DHIP(hipMemcpyAsync(&last[1], head + n - 1, 4, hipMemcpyDeviceToHost, s));
      DHIP(hipStreamSynchronize(s));
      const uint64_t nu = (uint64_t)last[0] + last[1];
      lap(3);
      // name ids and sums straight into the kept result; the per-query counts from the device
      hipLaunchKernelGGL(k_query_bounds, dim3(grid_of((uint64_t)nc + 1)), dim3(256), 0, s, out_key, nu, nc, d_qb);
      DHIP(hipGetLastError());
      const size_t at = c->batch_name.size();
      c->batch_name.resize(at + nu);
      c->batch_sum.resize(at + nu);
      qb.resize((size_t)nc + 1);
      DHIP(hipMemcpyAsync(c->batch_name.data() + at, out_name, nu * 4, hipMemcpyDeviceToHost, s));
      DHIP(hipMemcpyAsync(c->batch_sum.data() + at, out_sum, nu * 8, hipMemcpyDeviceToHost, s));
      DHIP(hipMemcpyAsync(qb.data(), d_qb, ((size_t)nc + 1) * 8, hipMemcpyDeviceToHost, s));
      DHIP(hipStreamSynchronize(s));
      for (uint32_t i = 0; i < nc; i++) c->batch_qoff[a + i + 1] = qb[i + 1] - qb[i];
      for (uint64_t i = 0; i < nu; i++) {
        const uint32_t id = c->batch_name[at + i];
        c->batch_name_bytes += c->name_off[id + 1] - c->name_off[id];
      }
      lap(4);
    }
    a = z;
  }
  for (uint32_t i = 0; i < n_q; i++) c->batch_qoff[i + 1] += c->batch_qoff[i];
  *n_out = c->batch_name.size();
  if (n_bytes) *n_bytes = c->batch_name_bytes;
  if (timing)
    fprintf(stderr, "shard batch %u, rank %d: first collective %.3f  local search %.3f  collectives %.3f  "
            "device merge %.3f  read-back %.3f ms\n", n_q, c->rank, t_stage[0], t_stage[1], t_stage[2], t_stage[3],
            t_stage[4]);
  return shard_partial(c, b.lrc, b.lmsg);
}

extern "C" int tfidf_dist_last_names_batch(const tfidf_comm *c, uint8_t *buf, uint64_t cap, uint64_t *offsets,
                                           double *scores, uint64_t n_cap, uint64_t *name_offsets, uint64_t *n_out,
                                           uint64_t *n_bytes) {
  if (!c || !name_offsets || !n_out || !n_bytes) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t n = c->batch_name.size();
  *n_out = n;
  *n_bytes = c->batch_name_bytes;
  for (size_t i = 0; i < c->batch_qoff.size(); i++) name_offsets[i] = c->batch_qoff[i];
  if (n > n_cap || c->batch_name_bytes > cap || (n && (!offsets || !scores)) || (c->batch_name_bytes && !buf))
    return errf(TFIDF_E_BUFFER, "%llu names of %llu bytes", (unsigned long long)n,
                (unsigned long long)c->batch_name_bytes);
  uint64_t p = 0;
  if (offsets) offsets[0] = 0;
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t id = c->batch_name[i];
    const uint64_t a = c->name_off[id], z = c->name_off[id + 1];
    memcpy(buf + p, c->names.data() + a, z - a);
    p += z - a;
    offsets[i + 1] = p;
    scores[i] = c->batch_sum[i];
  }
  return TFIDF_OK;
}

extern "C" int tfidf_dist_last_hits(const tfidf_comm *c, uint64_t *doc_ids, float *scores, uint64_t cap,
                                    uint64_t *n_out) {
  if (!c || !n_out) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  return write_hits(const_cast<tfidf_comm *>(c), doc_ids, scores, cap, n_out);
}

extern "C" int tfidf_dist_last_failed(const tfidf_comm *c, uint64_t *rank_mask) {
  if (!c || !rank_mask) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  *rank_mask = c->last_failed;
  return TFIDF_OK;
}

extern "C" int tfidf_dist_last_names(const tfidf_comm *c, uint8_t *buf, uint64_t cap, uint64_t *offsets,
                                     double *scores, uint64_t n_cap, uint64_t *n_out, uint64_t *n_bytes) {
  if (!c || !n_out || !n_bytes) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t n = c->last_name.size();
  *n_out = n;
  *n_bytes = c->last_name_bytes;
  if (n > n_cap || c->last_name_bytes > cap || (n && (!offsets || !scores)) || (c->last_name_bytes && !buf))
    return errf(TFIDF_E_BUFFER, "%llu names of %llu bytes", (unsigned long long)n,
                (unsigned long long)c->last_name_bytes);
  uint64_t p = 0;
  if (offsets) offsets[0] = 0;                     // (no names: the size query passes no arrays)
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t id = c->last_name[i];
    const uint64_t a = c->name_off[id], z = c->name_off[id + 1];
    memcpy(buf + p, c->names.data() + a, z - a);
    p += z - a;
    offsets[i + 1] = p;
    scores[i] = c->last_sum[i];
  }
  return TFIDF_OK;
}

// ---------------------------------------------------------------------------
// process model (1): one process, one shard per GPU

namespace {

// one persistent worker thread per shard: a node call runs the per-rank
// orchestration on every shard at once (the collectives need all ranks in flight)
struct ShardPool {
  std::vector<std::thread> th;
  std::mutex mu;
  std::condition_variable cv, done;
  std::function<int(uint32_t)> task;
  uint64_t gen = 0;
  uint32_t pending = 0;
  bool stop = false;
  std::vector<int> rc;
  std::vector<std::string> msg;
  explicit ShardPool(uint32_t n) : rc(n), msg(n) {
    for (uint32_t i = 0; i < n; i++)
      th.emplace_back([this, i] {
        uint64_t seen = 0;
        for (;;) {
          std::function<int(uint32_t)> f;
          {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return stop || gen != seen; });
            if (stop) return;
            seen = gen;
            f = task;
          }
          const int r = f(i);
          std::string m = r ? tfidf_last_error() : "";
          std::lock_guard<std::mutex> lk(mu);
          rc[i] = r;
          msg[i] = std::move(m);
          if (--pending == 0) done.notify_all();
        }
      });
  }
  ~ShardPool() {
    {
      std::lock_guard<std::mutex> lk(mu);
      stop = true;
    }
    cv.notify_all();
    for (auto &t : th) t.join();
  }
  // runs f(shard) on every shard; the first failure (lowest shard) is the result
  int run(std::function<int(uint32_t)> f) {
    {
      std::lock_guard<std::mutex> lk(mu);
      task = std::move(f);
      pending = (uint32_t)th.size();
      gen++;
    }
    cv.notify_all();
    std::unique_lock<std::mutex> lk(mu);
    done.wait(lk, [&] { return pending == 0; });
    for (size_t i = 0; i < rc.size(); i++)
      if (rc[i]) return set_error(rc[i], ("shard " + std::to_string(i) + ": " + msg[i]).c_str());
    return TFIDF_OK;
  }
};

}  // namespace

struct tfidf_node {
  tfidf_config cfg;
  std::vector<int> devices;
  std::vector<tfidf_index *> shards;
  std::vector<tfidf_comm *> comms;
  std::vector<uint64_t> doc_base;
  std::unique_ptr<ShardPool> pool;
  std::mutex mu;                     // node calls are serialised
  int transport = TFIDF_TRANSPORT_INPROC;
  bool committed = false;
  uint64_t num_docs = 0, doc_count = 0, sum_ttf = 0, num_terms = 0;
};

extern "C" int tfidf_node_create_devices(const tfidf_config *cfg, const int32_t *devices, uint32_t n_devices,
                                         uint32_t flags, tfidf_node **out) {
  if (!cfg || !devices || !out || n_devices == 0) return errf(TFIDF_E_INVALID_ARG, "NULL argument or no devices");
  if (n_devices > 64) return errf(TFIDF_E_INVALID_ARG, "at most 64 shards");
  std::unique_ptr<tfidf_node> n(new tfidf_node());
  n->cfg = *cfg;
  bool repeat = false;
  for (uint32_t i = 0; i < n_devices; i++) {
    for (uint32_t j = 0; j < i; j++) repeat |= devices[j] == devices[i];
    n->devices.push_back(devices[i]);
  }
  const bool inproc = repeat || (flags & TFIDF_NODE_INPROC);
  for (uint32_t i = 0; i < n_devices; i++) {
    tfidf_config c = *cfg;
    c.device = devices[i];
    tfidf_index *ix = nullptr;
    if (int rc = tfidf_create(&c, &ix)) {
      for (tfidf_index *x : n->shards) tfidf_destroy(x);
      return rc;
    }
    n->shards.push_back(ix);
  }
  if (inproc) {
    n->comms.resize(n_devices);
    tfidf_comm_create_inproc((int32_t)n_devices, n->comms.data());
    for (uint32_t i = 0; i < n_devices; i++) n->comms[i]->device = devices[i];
    n->transport = TFIDF_TRANSPORT_INPROC;
  } else {
    RcclApi &api = rccl();
    int rc = api.ok ? TFIDF_OK : errf(TFIDF_E_NO_DEVICE, "%s", api.err.c_str());
    std::vector<ncclComm_t> cm(n_devices, nullptr);
    if (!rc) {
      ncclResult_t r = api.CommInitAll(cm.data(), (int)n_devices, devices);
      if (r != ncclSuccess) rc = errf(TFIDF_E_HIP, "ncclCommInitAll: %s", api.GetErrorString(r));
    }
    if (rc) {
      for (tfidf_index *x : n->shards) tfidf_destroy(x);
      return rc;
    }
    for (uint32_t i = 0; i < n_devices; i++) {
      tfidf_comm *c = new tfidf_comm();
      c->rank = (int)i;
      c->world = (int)n_devices;
      c->device = devices[i];
      c->t.reset(new RcclTransport(cm[i], (int)n_devices));
      n->comms.push_back(c);
    }
    n->transport = TFIDF_TRANSPORT_RCCL;
  }
  n->doc_base.assign(n_devices, 0);
  n->pool.reset(new ShardPool(n_devices));
  *out = n.release();
  return TFIDF_OK;
}

extern "C" int tfidf_node_create(const tfidf_config *cfg, uint64_t device_mask, tfidf_node **out) {
  std::vector<int32_t> dev;
  for (int i = 0; i < 64; i++)
    if ((device_mask >> i) & 1u) dev.push_back(i);
  if (dev.empty()) return errf(TFIDF_E_INVALID_ARG, "empty device mask");
  return tfidf_node_create_devices(cfg, dev.data(), (uint32_t)dev.size(), 0, out);
}

extern "C" int tfidf_node_destroy(tfidf_node *n) {
  if (!n) return TFIDF_OK;
  n->pool.reset();
  for (tfidf_comm *c : n->comms) {
    DevGuard g(n->devices[c->rank]);
    delete c;
  }
  for (tfidf_index *x : n->shards) tfidf_destroy(x);
  delete n;
  return TFIDF_OK;
}

extern "C" int tfidf_node_shard(tfidf_node *n, uint32_t i, tfidf_index **ix, uint32_t *n_shards) {
  if (!n) return errf(TFIDF_E_INVALID_ARG, "NULL node");
  if (n_shards) *n_shards = (uint32_t)n->shards.size();
  if (ix) {
    if (i >= n->shards.size()) return errf(TFIDF_E_INVALID_ARG, "shard %u out of range", i);
    *ix = n->shards[i];
  }
  return TFIDF_OK;
}

extern "C" int tfidf_node_add_docs(tfidf_node *n, int32_t shard, const uint8_t *utf8, const uint64_t *offsets,
                                   uint64_t n_docs, const uint8_t *keys, const uint64_t *key_offsets) {
  if (!n || !offsets) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(n->mu);
  const uint32_t G = (uint32_t)n->shards.size();
  if (shard >= (int32_t)G || shard < -1) return errf(TFIDF_E_INVALID_ARG, "shard %d out of range", shard);
  n->committed = false;
  if (shard >= 0) return tfidf_add_docs(n->shards[shard], utf8, offsets, n_docs, keys, key_offsets);
  // contiguous split: shard g takes documents [g N / G, (g + 1) N / G)
  return n->pool->run([&](uint32_t g) {
    const uint64_t lo = g * n_docs / G, hi = (g + 1) * n_docs / G;
    return tfidf_add_docs(n->shards[g], utf8, offsets + lo, hi - lo, keys, keys ? key_offsets + lo : nullptr);
  });
}

// Deletes and compactions only stage changes: every shard keeps serving the
// snapshot of the last tfidf_node_commit, so the node stays committed.
extern "C" int tfidf_node_delete_docs(tfidf_node *n, int32_t shard, const uint8_t *keys, const uint64_t *key_offsets,
                                      uint64_t n_keys, uint64_t *n_deleted) {
  if (n_deleted) *n_deleted = 0;
  if (!n || (n_keys && !key_offsets)) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(n->mu);
  const uint32_t G = (uint32_t)n->shards.size();
  if (shard >= (int32_t)G || shard < -1) return errf(TFIDF_E_INVALID_ARG, "shard %d out of range", shard);
  if (shard >= 0) return tfidf_delete_docs(n->shards[shard], keys, key_offsets, n_keys, n_deleted);
  // a name can live on several shards (Leader-routed uploads): ask every one
  std::vector<uint64_t> nd(G, 0);
  int rc = n->pool->run([&](uint32_t g) { return tfidf_delete_docs(n->shards[g], keys, key_offsets, n_keys, &nd[g]); });
  if (n_deleted)
    for (uint64_t v : nd) *n_deleted += v;
  return rc;
}

extern "C" int tfidf_node_compact(tfidf_node *n, uint64_t *bytes_reclaimed) {
  if (bytes_reclaimed) *bytes_reclaimed = 0;
  if (!n) return errf(TFIDF_E_INVALID_ARG, "NULL node");
  std::lock_guard<std::mutex> lk(n->mu);
  std::vector<uint64_t> nb(n->shards.size(), 0);
  int rc = n->pool->run([&](uint32_t g) { return tfidf_compact(n->shards[g], &nb[g], nullptr); });
  if (bytes_reclaimed)
    for (uint64_t v : nb) *bytes_reclaimed += v;
  return rc;
}

extern "C" int tfidf_node_commit(tfidf_node *n) {
  if (!n) return errf(TFIDF_E_INVALID_ARG, "NULL node");
  std::lock_guard<std::mutex> lk(n->mu);
  n->committed = false;
  // 1. every shard's own commit (all of them, before any collective: a shard
  //    that fails must not leave the others waiting in an exchange)
  if (int rc = n->pool->run([&](uint32_t g) { return tfidf_commit(n->shards[g]); })) return rc;
  uint64_t base = 0, dc = 0, ttf = 0;
  for (size_t g = 0; g < n->shards.size(); g++) {
    tfidf_index_stats st{};
    if (int rc = tfidf_stats(n->shards[g], &st)) return rc;
    n->doc_base[g] = base;
    base += st.num_docs;
    dc += st.doc_count;
    ttf += st.sum_ttf;
  }
  if (base > (1ull << 32)) return errf(TFIDF_E_CAPACITY, "more than 2^32 documents on the node");
  n->num_docs = base;
  // 2. GLOBAL statistics, or the SHARD name table
  if (n->cfg.stats_mode == TFIDF_STATS_GLOBAL) {
    std::vector<uint64_t> nv(n->shards.size()), gdc(n->shards.size()), gttf(n->shards.size());
    if (int rc = n->pool->run([&](uint32_t g) {
          return tfidf_dist_global_commit(n->shards[g], n->comms[g], &nv[g], &gdc[g], &gttf[g]);
        }))
      return rc;
    n->num_terms = nv[0];
    n->doc_count = gdc[0];
    n->sum_ttf = gttf[0];
  } else {
    if (int rc = n->pool->run([&](uint32_t g) { return tfidf_dist_shard_commit(n->shards[g], n->comms[g], nullptr); }))
      return rc;
    n->num_terms = 0;
    n->doc_count = dc;
    n->sum_ttf = ttf;
  }
  n->committed = true;
  return TFIDF_OK;
}

extern "C" int tfidf_node_search(tfidf_node *n, const uint8_t *q, uint64_t q_len, uint32_t k, uint64_t *doc_ids,
                                 float *scores, uint64_t cap, uint64_t *n_out) {
  if (!n || !n_out) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(n->mu);
  *n_out = 0;
  if (!n->committed) return errf(TFIDF_E_STATE, "search before tfidf_node_commit");
  if (n->cfg.stats_mode != TFIDF_STATS_GLOBAL) return errf(TFIDF_E_STATE, "GLOBAL mode only (tfidf_node_search_names)");
  if (int rc = n->pool->run([&](uint32_t g) {
        uint64_t m = 0;
        const int r = tfidf_dist_search(n->shards[g], n->comms[g], n->doc_base[g], q, q_len, k, nullptr, nullptr, 0, &m);
        return r == TFIDF_E_BUFFER ? TFIDF_OK : r;
      }))
    return rc;
  return write_hits(n->comms[0], doc_ids, scores, cap, n_out);
}

extern "C" int tfidf_node_search_batch(tfidf_node *n, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                                       uint32_t k, uint64_t *doc_ids, float *scores, uint32_t *counts) {
  if (!n) return errf(TFIDF_E_INVALID_ARG, "NULL node");
  std::lock_guard<std::mutex> lk(n->mu);
  if (!n->committed) return errf(TFIDF_E_STATE, "search before tfidf_node_commit");
  if (n->cfg.stats_mode != TFIDF_STATS_GLOBAL) return errf(TFIDF_E_STATE, "GLOBAL mode only");
  if (k == 0 || k > 1024) return errf(TFIDF_E_INVALID_ARG, "1 <= k <= 1024");
  const size_t per = (size_t)n_q * k;
  std::vector<std::vector<uint64_t>> d(n->shards.size());
  std::vector<std::vector<float>> sc(n->shards.size());
  std::vector<std::vector<uint32_t>> ct(n->shards.size());
  // shard 0 writes the caller's arrays; the others' (identical) copies are scratch
  return n->pool->run([&](uint32_t g) {
    uint64_t *pd = doc_ids;
    float *ps = scores;
    uint32_t *pc = counts;
    if (g) {
      d[g].resize(per);
      sc[g].resize(per);
      ct[g].resize(n_q);
      pd = d[g].data();
      ps = sc[g].data();
      pc = ct[g].data();
    }
    return tfidf_dist_search_batch(n->shards[g], n->comms[g], n->doc_base[g], q_utf8, q_offsets, n_q, k, pd, ps, pc);
  });
}

extern "C" int tfidf_node_search_names(tfidf_node *n, const uint8_t *q, uint64_t q_len, uint8_t *buf, uint64_t cap,
                                       uint64_t *offsets, double *scores, uint64_t n_cap, uint64_t *n_out,
                                       uint64_t *n_bytes) {
  if (!n || !n_out || !n_bytes) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(n->mu);
  *n_out = *n_bytes = 0;
  if (!n->committed) return errf(TFIDF_E_STATE, "search before tfidf_node_commit");
  if (n->cfg.stats_mode != TFIDF_STATS_SHARD) return errf(TFIDF_E_STATE, "SHARD mode only (tfidf_node_search)");
  std::vector<std::string> why(n->shards.size());
  if (int rc = n->pool->run([&](uint32_t g) {
        uint64_t m = 0, b = 0;
        const int r = tfidf_dist_shard_search(n->shards[g], n->comms[g], q, q_len, &m, &b);
        if (r == TFIDF_OK && n->comms[g]->last_failed) why[g] = tfidf_last_error();
        return r;
      }))
    return rc;
  const int rc = tfidf_dist_last_names(n->comms[0], buf, cap, offsets, scores, n_cap, n_out, n_bytes);
  if (rc == TFIDF_OK && n->comms[0]->last_failed) {        // partial answer: say which shards were skipped
    std::string m = why[0];
    for (size_t g = 0; g < why.size(); g++)
      if ((n->comms[0]->last_failed >> g) & 1u) m += "; shard " + std::to_string(g) + ": " + why[g];
    set_error(TFIDF_OK, m.c_str());
  }
  return rc;
}

extern "C" int tfidf_node_search_batch_all(tfidf_node *n, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                                           uint64_t *doc_ids, float *scores, uint64_t cap, uint64_t *hit_offsets,
                                           uint64_t *n_out) {
  if (!n || !hit_offsets || !n_out || (n_q && !q_offsets) || (cap && (!doc_ids || !scores)))
    return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(n->mu);
  for (uint32_t i = 0; i <= n_q; i++) hit_offsets[i] = 0;
  *n_out = 0;
  if (!n->committed) return errf(TFIDF_E_STATE, "search before tfidf_node_commit");
  if (n->cfg.stats_mode != TFIDF_STATS_GLOBAL)
    return errf(TFIDF_E_STATE, "GLOBAL mode only (tfidf_node_search_names_batch)");
  // shard 0 writes the caller's arrays; the others take part with cap == 0 (offsets only)
  std::vector<std::vector<uint64_t>> ho(n->shards.size());
  int rc0 = TFIDF_OK;
  std::string msg0;
  const int rc = n->pool->run([&](uint32_t g) {
    if (g == 0) {
      rc0 = tfidf_dist_search_batch_all(n->shards[0], n->comms[0], n->doc_base[0], q_utf8, q_offsets, n_q, doc_ids,
                                        scores, cap, hit_offsets, n_out);
      if (rc0 == TFIDF_E_BUFFER) msg0 = tfidf_last_error();
      return rc0 == TFIDF_E_BUFFER ? TFIDF_OK : rc0;
    }
    ho[g].assign((size_t)n_q + 1, 0);
    uint64_t m = 0;
    const int r = tfidf_dist_search_batch_all(n->shards[g], n->comms[g], n->doc_base[g], q_utf8, q_offsets, n_q,
                                              nullptr, nullptr, 0, ho[g].data(), &m);
    return r == TFIDF_E_BUFFER ? TFIDF_OK : r;
  });
  if (rc) return rc;
  return rc0 == TFIDF_E_BUFFER ? set_error(TFIDF_E_BUFFER, msg0.c_str()) : TFIDF_OK;
}

extern "C" int tfidf_node_search_names_batch(tfidf_node *n, const uint8_t *q_utf8, const uint64_t *q_offsets,
                                             uint32_t n_q, uint64_t *n_out, uint64_t *n_bytes) {
  if (!n || !n_out || (n_q && !q_offsets)) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(n->mu);
  *n_out = 0;
  if (n_bytes) *n_bytes = 0;
  if (!n->committed) return errf(TFIDF_E_STATE, "search before tfidf_node_commit");
  if (n->cfg.stats_mode != TFIDF_STATS_SHARD)
    return errf(TFIDF_E_STATE, "SHARD mode only (tfidf_node_search_batch_all)");
  std::vector<std::string> why(n->shards.size());
  std::vector<uint64_t> m(n->shards.size(), 0), b(n->shards.size(), 0);
  if (int rc = n->pool->run([&](uint32_t g) {
        const int r = tfidf_dist_shard_search_batch(n->shards[g], n->comms[g], q_utf8, q_offsets, n_q, &m[g], &b[g]);
        if (r == TFIDF_OK && n->comms[g]->last_failed) why[g] = tfidf_last_error();
        return r;
      }))
    return rc;
  *n_out = m[0];
  if (n_bytes) *n_bytes = b[0];
  if (n->comms[0]->last_failed) {                          // partial answer: say which shards were skipped
    std::string msg = why[0];
    for (size_t g = 0; g < why.size(); g++)
      if ((n->comms[0]->last_failed >> g) & 1u) msg += "; shard " + std::to_string(g) + ": " + why[g];
    set_error(TFIDF_OK, msg.c_str());
  }
  return TFIDF_OK;
}

extern "C" int tfidf_node_last_names_batch(const tfidf_node *n, uint8_t *buf, uint64_t cap, uint64_t *offsets,
                                           double *scores, uint64_t n_cap, uint64_t *name_offsets, uint64_t *n_out,
                                           uint64_t *n_bytes) {
  if (!n || !name_offsets || !n_out || !n_bytes) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(const_cast<tfidf_node *>(n)->mu);
  return tfidf_dist_last_names_batch(n->comms[0], buf, cap, offsets, scores, n_cap, name_offsets, n_out, n_bytes);
}

extern "C" int tfidf_node_last_failed(const tfidf_node *n, uint64_t *shard_mask) {
  if (!n || !shard_mask) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  *shard_mask = n->comms.empty() ? 0 : n->comms[0]->last_failed;
  return TFIDF_OK;
}

extern "C" int tfidf_node_doc_key(tfidf_node *n, uint64_t doc, uint8_t *buf, uint64_t cap, uint64_t *n_out) {
  if (!n || !n_out) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(n->mu);
  if (!n->committed) return errf(TFIDF_E_STATE, "not committed");
  if (doc >= n->num_docs) return errf(TFIDF_E_INVALID_ARG, "doc out of range");
  size_t g = n->shards.size() - 1;
  while (n->doc_base[g] > doc) g--;
  return tfidf_doc_key(n->shards[g], doc - n->doc_base[g], buf, cap, n_out);
}

// ---------------------------------------------------------------------------
// batched hit highlighting over the node: rows by global doc id

namespace {

struct NodeHlOut {                     // the caller's arrays (HlOut of tfidf_capi.hip, global rows)
  uint32_t W = 0;                      // 0 = matches
  uint8_t *text = nullptr;
  uint64_t text_cap = 0;
  uint64_t *text_offsets = nullptr, *doc_starts = nullptr, *n_text = nullptr;
  uint64_t *starts = nullptr;
  uint32_t *lens = nullptr, *ordinals = nullptr;
  uint64_t m_cap = 0;
  uint64_t *match_offsets = nullptr, *n_matches = nullptr;
  float *ms_device = nullptr;
};

struct ShardRows {                     // one shard's batch: its rows in the caller's order
  std::vector<uint64_t> row;           // caller row of local row j
  std::vector<uint32_t> docs;          // shard-local doc ids
  std::vector<uint64_t> doc_offsets;   // n_q + 1
  std::vector<uint8_t> text;
  std::vector<uint64_t> text_offsets, doc_starts, starts, match_offsets;
  std::vector<uint32_t> lens, ordinals;
  float ms = 0.0f;
};

// one shard's batch: once with guessed payload sizes, once more with the sizes it reports
int shard_highlight(tfidf_index *ix, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q, uint32_t W,
                    ShardRows &b) {
  const uint64_t R = b.docs.size();
  b.match_offsets.assign(R + 1, 0);
  b.text_offsets.assign(R + 1, 0);
  b.doc_starts.assign(R, 0);
  uint64_t t_cap = W ? std::min<uint64_t>(R * W, 64ull << 20) : 0, m_cap = 64 * R, nt = 0, nm = 0;
  int rc = TFIDF_OK;
  for (int attempt = 0; attempt < 2; attempt++) {
    b.text.resize(t_cap);
    b.starts.resize(m_cap);
    b.lens.resize(m_cap);
    b.ordinals.resize(m_cap);
    rc = W ? tfidf_snippets_batch(ix, q_utf8, q_offsets, n_q, b.docs.data(), b.doc_offsets.data(), W, b.text.data(),
                                  t_cap, b.text_offsets.data(), b.doc_starts.data(), b.starts.data(), b.lens.data(),
                                  b.ordinals.data(), m_cap, b.match_offsets.data(), &nt, &nm, &b.ms)
           : tfidf_matches_batch(ix, q_utf8, q_offsets, n_q, b.docs.data(), b.doc_offsets.data(), b.starts.data(),
                                 b.lens.data(), b.ordinals.data(), m_cap, b.match_offsets.data(), &nm, &b.ms);
    if (rc != TFIDF_E_BUFFER) break;
    t_cap = nt;
    m_cap = nm;
  }
  return rc;
}

int node_highlight(tfidf_node *n, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q, const uint64_t *docs,
                   const uint64_t *doc_offsets, const NodeHlOut &o) {
  std::lock_guard<std::mutex> lk(n->mu);
  if (o.ms_device) *o.ms_device = 0.0f;
  if (!n->committed) return errf(TFIDF_E_STATE, "highlighting before tfidf_node_commit");
  if (doc_offsets[0] != 0) return errf(TFIDF_E_INVALID_ARG, "doc_offsets[0] is not 0");
  for (uint32_t i = 0; i < n_q; i++)
    if (doc_offsets[i + 1] < doc_offsets[i]) return errf(TFIDF_E_INVALID_ARG, "doc_offsets decrease at query %u", i);
  const uint64_t R = doc_offsets[n_q];
  if (R > (1ull << 26)) return errf(TFIDF_E_INVALID_ARG, "more than 2^26 rows in one call");
  for (uint64_t r = 0; r < R; r++)
    if (docs[r] >= n->num_docs)
      return errf(TFIDF_E_INVALID_ARG, "doc %llu out of range", (unsigned long long)docs[r]);
  // rows to their shards (tfidf_node_doc_key's rule), query grouping and order kept
  const size_t G = n->shards.size();
  std::vector<ShardRows> sh(G);
  std::vector<uint32_t> row_shard(R);
  std::vector<uint64_t> row_local(R);
  for (size_t g = 0; g < G; g++) sh[g].doc_offsets.assign((size_t)n_q + 1, 0);
  for (uint32_t i = 0; i < n_q; i++) {
    for (uint64_t r = doc_offsets[i]; r < doc_offsets[i + 1]; r++) {
      size_t g = G - 1;
      while (n->doc_base[g] > docs[r]) g--;
      row_shard[r] = (uint32_t)g;
      row_local[r] = sh[g].docs.size();
      sh[g].row.push_back(r);
      sh[g].docs.push_back((uint32_t)(docs[r] - n->doc_base[g]));
    }
    for (size_t g = 0; g < G; g++) sh[g].doc_offsets[i + 1] = sh[g].docs.size();
  }
  // every shard with rows runs its own batch at once
  if (int rc = n->pool->run([&](uint32_t g) {
        return sh[g].docs.empty() ? TFIDF_OK : shard_highlight(n->shards[g], q_utf8, q_offsets, n_q, o.W, sh[g]);
      }))
    return rc;
  // back into the caller's row order: offsets first (always in full), then the payload when it fits
  uint64_t nt = 0, nm = 0;
  o.match_offsets[0] = 0;
  if (o.W) o.text_offsets[0] = 0;
  for (uint64_t r = 0; r < R; r++) {
    const ShardRows &b = sh[row_shard[r]];
    const uint64_t j = row_local[r];
    nm += b.match_offsets[j + 1] - b.match_offsets[j];
    o.match_offsets[r + 1] = nm;
    if (o.W) {
      nt += b.text_offsets[j + 1] - b.text_offsets[j];
      o.text_offsets[r + 1] = nt;
      o.doc_starts[r] = b.doc_starts[j];
    }
  }
  *o.n_matches = nm;
  if (o.W) *o.n_text = nt;
  if (o.ms_device)
    for (const ShardRows &b : sh) *o.ms_device = std::max(*o.ms_device, b.ms);
  if (nm > o.m_cap || (nm && (!o.starts || !o.lens || !o.ordinals)) || (o.W && (nt > o.text_cap || (nt && !o.text))))
    return errf(TFIDF_E_BUFFER, "need %llu text bytes and %llu match slots", (unsigned long long)nt,
                (unsigned long long)nm);
  for (uint64_t r = 0; r < R; r++) {
    const ShardRows &b = sh[row_shard[r]];
    const uint64_t j = row_local[r], m0 = b.match_offsets[j], mc = b.match_offsets[j + 1] - m0;
    if (mc) {
      memcpy(o.starts + o.match_offsets[r], b.starts.data() + m0, mc * 8);
      memcpy(o.lens + o.match_offsets[r], b.lens.data() + m0, mc * 4);
      memcpy(o.ordinals + o.match_offsets[r], b.ordinals.data() + m0, mc * 4);
    }
    if (o.W && b.text_offsets[j + 1] > b.text_offsets[j])
      memcpy(o.text + o.text_offsets[r], b.text.data() + b.text_offsets[j], b.text_offsets[j + 1] - b.text_offsets[j]);
  }
  return TFIDF_OK;
}

}  // namespace

extern "C" int tfidf_node_matches_batch(tfidf_node *n, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                                        const uint64_t *docs, const uint64_t *doc_offsets, uint64_t *starts,
                                        uint32_t *lens, uint32_t *ordinals, uint64_t cap, uint64_t *match_offsets,
                                        uint64_t *n_out, float *ms_device) {
  if (!n || (n_q && !q_offsets) || !doc_offsets || (!docs && doc_offsets[n_q]) || !match_offsets || !n_out)
    return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  NodeHlOut o;
  o.starts = starts;
  o.lens = lens;
  o.ordinals = ordinals;
  o.m_cap = cap;
  o.match_offsets = match_offsets;
  o.n_matches = n_out;
  o.ms_device = ms_device;
  return node_highlight(n, q_utf8, q_offsets, n_q, docs, doc_offsets, o);
}

extern "C" int tfidf_node_snippets_batch(tfidf_node *n, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                                         const uint64_t *docs, const uint64_t *doc_offsets, uint32_t max_bytes,
                                         uint8_t *text, uint64_t text_cap, uint64_t *text_offsets,
                                         uint64_t *doc_starts, uint64_t *starts, uint32_t *lens, uint32_t *ordinals,
                                         uint64_t m_cap, uint64_t *match_offsets, uint64_t *n_text,
                                         uint64_t *n_matches, float *ms_device) {
  if (!n || (n_q && !q_offsets) || !doc_offsets || (!docs && doc_offsets[n_q]) || !text_offsets ||
      (!doc_starts && doc_offsets[n_q]) || !match_offsets || !n_text || !n_matches)
    return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  if (max_bytes < 16 || max_bytes > 65536)
    return errf(TFIDF_E_INVALID_ARG, "max_bytes %u outside 16..65536", max_bytes);
  NodeHlOut o;
  o.W = max_bytes;
  o.text = text;
  o.text_cap = text_cap;
  o.text_offsets = text_offsets;
  o.doc_starts = doc_starts;
  o.n_text = n_text;
  o.starts = starts;
  o.lens = lens;
  o.ordinals = ordinals;
  o.m_cap = m_cap;
  o.match_offsets = match_offsets;
  o.n_matches = n_matches;
  o.ms_device = ms_device;
  return node_highlight(n, q_utf8, q_offsets, n_q, docs, doc_offsets, o);
}

// ---------------------------------------------------------------------------
// fuzzy term lookup over the node: every shard's untruncated candidates, merged by term bytes

extern "C" int tfidf_node_fuzzy_terms_batch(tfidf_node *n, const uint8_t *t_utf8, const uint64_t *t_offsets,
                                            uint32_t n_terms, uint32_t max_edits, uint32_t prefix_len,
                                            uint32_t max_out, uint64_t *cand_offsets, uint64_t *n_within,
                                            uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap, uint64_t *df,
                                            uint8_t *dist, uint64_t cand_cap, uint64_t *n_cands,
                                            uint64_t *n_term_bytes, float *ms_device) {
  if (!n || !cand_offsets || (n_terms && (!n_within || !t_offsets)) || !n_cands || !n_term_bytes)
    return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  if (max_out < 1 || max_out > 1024) return errf(TFIDF_E_INVALID_ARG, "max_out %u outside 1..1024", max_out);
  if (max_edits > 2) return errf(TFIDF_E_INVALID_ARG, "max_edits %u above 2", max_edits);
  if (n_terms > 65536) return errf(TFIDF_E_INVALID_ARG, "more than 65536 terms in one call");
  std::lock_guard<std::mutex> lk(n->mu);
  if (ms_device) *ms_device = 0.0f;
  if (!n->committed) return errf(TFIDF_E_STATE, "fuzzy lookup before tfidf_node_commit");
  const size_t G = n->shards.size();
  std::vector<FuzzyLists> sh(G);
  if (int rc = n->pool->run([&](uint32_t g) {
        return index_fuzzy_terms(n->shards[g], t_utf8, t_offsets, n_terms, max_edits, prefix_len, 0, &sh[g]);
      }))
    return rc;
  // per input term: the shards' candidates by term bytes (df summed), then the order of the single index
  std::vector<std::vector<FuzzyCand>> merged(n_terms);
  uint64_t nc = 0, nb = 0;
  cand_offsets[0] = 0;
  for (uint32_t i = 0; i < n_terms; i++) {
    std::map<std::string, FuzzyCand> by;
    for (size_t g = 0; g < G; g++)
      for (const FuzzyCand &c : sh[g].cands[i]) {
        auto it = by.find(c.term);
        if (it == by.end()) by.emplace(c.term, c);
        else it->second.df += c.df;
      }
    std::vector<FuzzyCand> &L = merged[i];
    for (auto &kv : by) L.push_back(kv.second);
    std::sort(L.begin(), L.end(), [](const FuzzyCand &x, const FuzzyCand &y) {
      if (x.dist != y.dist) return x.dist < y.dist;
      if (x.df != y.df) return x.df > y.df;
      return x.term < y.term;
    });
    n_within[i] = L.size();
    if (L.size() > max_out) L.resize(max_out);
    nc += L.size();
    for (const FuzzyCand &c : L) nb += c.term.size();
    cand_offsets[i + 1] = nc;
  }
  *n_cands = nc;
  *n_term_bytes = nb;
  if (ms_device)
    for (const FuzzyLists &f : sh) *ms_device = std::max(*ms_device, f.ms_device);
  if (nc > cand_cap || nb > terms_cap || (nc && (!term_offsets || !df || !dist)) || (nb && !terms))
    return errf(TFIDF_E_BUFFER, "need %llu candidate slots and %llu term bytes", (unsigned long long)nc,
                (unsigned long long)nb);
  uint64_t at = 0, b = 0;
  if (term_offsets) term_offsets[0] = 0;
  for (uint32_t i = 0; i < n_terms; i++)
    for (const FuzzyCand &c : merged[i]) {
      memcpy(terms + b, c.term.data(), c.term.size());
      b += c.term.size();
      df[at] = c.df;
      dist[at] = (uint8_t)c.dist;
      term_offsets[++at] = b;
    }
  return TFIDF_OK;
}

// ---------------------------------------------------------------------------
// wildcard and regex search over the node: every shard's untruncated term lists
// merged by term bytes; the shards' ascending hit lists put one after the other

// tabs: the compiled tables of a regex call (compiled once for every shard and pass), NULL for a wildcard call
static int node_multiterm_run(tfidf_node *n, const std::vector<std::vector<uint32_t>> *tabs, const uint8_t *p_utf8,
                              const uint64_t *p_offsets, uint32_t n_p, bool docs, std::vector<WildcardLists> *sh,
                              std::vector<uint8_t> *ran) {
  const size_t G = n->shards.size();
  sh->assign(G, {});
  ran->assign(G, 0);
  return n->pool->run([&](uint32_t g) {
    tfidf_index *ix = n->shards[g];
    if (!index_committed(ix) || index_num_docs(ix) == 0) return (int)TFIDF_OK;
    const int rc = tabs ? index_regex(ix, *tabs, docs, 0, &(*sh)[g])
                        : index_wildcard(ix, p_utf8, p_offsets, n_p, docs, 0, &(*sh)[g]);
    (*ran)[g] = rc == TFIDF_OK;
    return rc;
  });
}

// pattern i's terms over the shards by term bytes (df summed), in the order of the single index
static void node_multiterm_merge(const std::vector<WildcardLists> &sh, const std::vector<uint8_t> &ran, uint32_t i,
                                std::vector<FuzzyCand> *L) {
  std::map<std::string, FuzzyCand> by;
  for (size_t g = 0; g < sh.size(); g++) {
    if (!ran[g]) continue;
    for (const FuzzyCand &c : sh[g].terms[i]) {
      auto it = by.find(c.term);
      if (it == by.end()) by.emplace(c.term, c);
      else it->second.df += c.df;
    }
  }
  L->clear();
  for (auto &kv : by) L->push_back(kv.second);
  std::sort(L->begin(), L->end(), [](const FuzzyCand &x, const FuzzyCand &y) {
    if (x.df != y.df) return x.df > y.df;
    return x.term < y.term;
  });
}

static int node_multiterm_args(const tfidf_node *n, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p) {
  if (!n || (n_p && (!p_offsets || (!p_utf8 && p_offsets[n_p] != p_offsets[0]))))
    return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  if (n_p > 65536) return errf(TFIDF_E_INVALID_ARG, "more than 65536 patterns in one call");
  for (uint32_t i = 0; i < n_p; i++)
    if (p_offsets[i + 1] < p_offsets[i]) return errf(TFIDF_E_INVALID_ARG, "p_offsets decrease at pattern %u", i);
  return TFIDF_OK;
}

static int node_multiterm_terms(tfidf_node *n, bool regex, const uint8_t *p_utf8, const uint64_t *p_offsets,
                               uint32_t n_p, uint32_t max_out, uint64_t *cand_offsets, uint64_t *n_matched,
                               uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap, uint64_t *df,
                               uint64_t cand_cap, uint64_t *n_cands, uint64_t *n_term_bytes, float *ms_device) {
  const char *const what = regex ? "regex" : "wildcard";
  if (int rc = node_multiterm_args(n, p_utf8, p_offsets, n_p)) return rc;
  if (!cand_offsets || (n_p && !n_matched) || !n_cands || !n_term_bytes) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  if (max_out < 1 || max_out > 1024) return errf(TFIDF_E_INVALID_ARG, "max_out %u outside 1..1024", max_out);
  std::vector<std::vector<uint32_t>> tabs;       // a pattern in error fails the call before any shard runs
  if (regex)
    if (int rc = regex_compile_all(p_utf8, p_offsets, n_p, &tabs)) return rc;
  std::lock_guard<std::mutex> lk(n->mu);
  if (ms_device) *ms_device = 0.0f;
  if (!n->committed) return errf(TFIDF_E_STATE, "%s lookup before tfidf_node_commit", what);
  std::vector<WildcardLists> sh;
  std::vector<uint8_t> ran;
  if (int rc = node_multiterm_run(n, regex ? &tabs : nullptr, p_utf8, p_offsets, n_p, false, &sh, &ran)) return rc;
  std::vector<std::vector<FuzzyCand>> merged(n_p);
  uint64_t nc = 0, nb = 0;
  cand_offsets[0] = 0;
  for (uint32_t i = 0; i < n_p; i++) {
    std::vector<FuzzyCand> &L = merged[i];
    node_multiterm_merge(sh, ran, i, &L);
    n_matched[i] = L.size();
    if (L.size() > max_out) L.resize(max_out);
    nc += L.size();
    for (const FuzzyCand &c : L) nb += c.term.size();
    cand_offsets[i + 1] = nc;
  }
  *n_cands = nc;
  *n_term_bytes = nb;
  if (ms_device)
    for (const WildcardLists &w : sh) *ms_device = std::max(*ms_device, w.ms_device);
  if (nc > cand_cap || nb > terms_cap || (nc && (!term_offsets || !df)) || (nb && !terms))
    return errf(TFIDF_E_BUFFER, "need %llu term slots and %llu term bytes", (unsigned long long)nc,
                (unsigned long long)nb);
  uint64_t at = 0, b = 0;
  if (term_offsets) term_offsets[0] = 0;
  for (uint32_t i = 0; i < n_p; i++)
    for (const FuzzyCand &c : merged[i]) {
      memcpy(terms + b, c.term.data(), c.term.size());
      b += c.term.size();
      df[at] = c.df;
      term_offsets[++at] = b;
    }
  return TFIDF_OK;
}

extern "C" int tfidf_node_wildcard_terms_batch(tfidf_node *n, const uint8_t *p_utf8, const uint64_t *p_offsets,
                                               uint32_t n_p, uint32_t max_out, uint64_t *cand_offsets,
                                               uint64_t *n_matched, uint64_t *term_offsets, uint8_t *terms,
                                               uint64_t terms_cap, uint64_t *df, uint64_t cand_cap, uint64_t *n_cands,
                                               uint64_t *n_term_bytes, float *ms_device) {
  return node_multiterm_terms(n, false, p_utf8, p_offsets, n_p, max_out, cand_offsets, n_matched, term_offsets, terms,
                             terms_cap, df, cand_cap, n_cands, n_term_bytes, ms_device);
}

extern "C" int tfidf_node_regex_terms_batch(tfidf_node *n, const uint8_t *p_utf8, const uint64_t *p_offsets,
                                            uint32_t n_p, uint32_t max_out, uint64_t *cand_offsets,
                                            uint64_t *n_matched, uint64_t *term_offsets, uint8_t *terms,
                                            uint64_t terms_cap, uint64_t *df, uint64_t cand_cap, uint64_t *n_cands,
                                            uint64_t *n_term_bytes, float *ms_device) {
  return node_multiterm_terms(n, true, p_utf8, p_offsets, n_p, max_out, cand_offsets, n_matched, term_offsets, terms,
                             terms_cap, df, cand_cap, n_cands, n_term_bytes, ms_device);
}

static int node_multiterm_docs(tfidf_node *n, bool regex, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p,
                              uint64_t *doc_ids, uint64_t cap, uint64_t *hit_offsets, uint64_t *n_matched,
                              uint64_t *n_out, float *ms_device) {
  if (int rc = node_multiterm_args(n, p_utf8, p_offsets, n_p)) return rc;
  if (!hit_offsets || (n_p && !n_matched) || !n_out) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  std::vector<std::vector<uint32_t>> tabs;       // a pattern in error fails the call before any shard runs
  if (regex)
    if (int rc = regex_compile_all(p_utf8, p_offsets, n_p, &tabs)) return rc;
  std::lock_guard<std::mutex> lk(n->mu);
  if (ms_device) *ms_device = 0.0f;
  if (!n->committed) return errf(TFIDF_E_STATE, "%s search before tfidf_node_commit", regex ? "regex" : "wildcard");
  const size_t G = n->shards.size();
  std::vector<WildcardLists> sh, tsh;
  std::vector<uint8_t> ran, tran;
  if (int rc = node_multiterm_run(n, regex ? &tabs : nullptr, p_utf8, p_offsets, n_p, true, &sh, &ran)) return rc;
  // the distinct matching terms need the shards' term strings when more than one shard ran
  size_t n_ran = 0;
  for (size_t g = 0; g < G; g++) n_ran += ran[g];
  if (n_ran > 1)
    if (int rc = node_multiterm_run(n, regex ? &tabs : nullptr, p_utf8, p_offsets, n_p, false, &tsh, &tran)) return rc;
  std::vector<FuzzyCand> L;
  uint64_t total = 0;
  hit_offsets[0] = 0;
  for (uint32_t i = 0; i < n_p; i++) {
    n_matched[i] = 0;
    if (n_ran > 1) {
      node_multiterm_merge(tsh, tran, i, &L);
      n_matched[i] = L.size();
    }
    for (size_t g = 0; g < G; g++) {
      if (!ran[g]) continue;
      if (n_ran == 1) n_matched[i] = sh[g].n_matched[i];
      total += sh[g].hit_off[i + 1] - sh[g].hit_off[i];
    }
    hit_offsets[i + 1] = total;
  }
  *n_out = total;
  if (ms_device) {
    for (const WildcardLists &w : sh) *ms_device = std::max(*ms_device, w.ms_device);
    for (const WildcardLists &w : tsh) *ms_device = std::max(*ms_device, w.ms_device);
  }
  if (total > cap || (total && !doc_ids)) return errf(TFIDF_E_BUFFER, "need %llu hit slots", (unsigned long long)total);
  uint64_t o = 0;
  for (uint32_t i = 0; i < n_p; i++)
    for (size_t g = 0; g < G; g++) {
      if (!ran[g]) continue;
      for (uint64_t j = sh[g].hit_off[i]; j < sh[g].hit_off[i + 1]; j++) doc_ids[o++] = n->doc_base[g] + sh[g].docs[j];
    }
  return TFIDF_OK;
}

extern "C" int tfidf_node_search_wildcard_batch(tfidf_node *n, const uint8_t *p_utf8, const uint64_t *p_offsets,
                                                uint32_t n_p, uint64_t *doc_ids, uint64_t cap, uint64_t *hit_offsets,
                                                uint64_t *n_matched, uint64_t *n_out, float *ms_device) {
  return node_multiterm_docs(n, false, p_utf8, p_offsets, n_p, doc_ids, cap, hit_offsets, n_matched, n_out, ms_device);
}

extern "C" int tfidf_node_search_regex_batch(tfidf_node *n, const uint8_t *p_utf8, const uint64_t *p_offsets,
                                             uint32_t n_p, uint64_t *doc_ids, uint64_t cap, uint64_t *hit_offsets,
                                             uint64_t *n_matched, uint64_t *n_out, float *ms_device) {
  return node_multiterm_docs(n, true, p_utf8, p_offsets, n_p, doc_ids, cap, hit_offsets, n_matched, n_out, ms_device);
}

// ---------------------------------------------------------------------------
// exact phrase search over the node: every shard's ordered hits, merged per
// phrase by (score descending, global id ascending).  slops == nullptr: the
// exact call, freqs are counts; else tfidf_search_phrase_slop_batch per shard,
// freqs are the words of float frequencies.

static int node_phrase_batch(tfidf_node *n, const uint8_t *p_utf8, const uint64_t *p_offsets, const uint32_t *slops,
                             bool sloppy, uint32_t n_p, uint64_t *doc_ids, float *scores, uint32_t *freqs,
                             uint64_t cap, uint64_t *hit_offsets, uint64_t *n_out) {
  if (!n || !hit_offsets || !n_out || (n_p && (!p_offsets || (!p_utf8 && p_offsets[n_p]))) ||
      (cap && (!doc_ids || !scores || !freqs)) || (sloppy && n_p && !slops))
    return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(n->mu);
  if (!n->committed) return errf(TFIDF_E_STATE, "phrase search before tfidf_node_commit");
  struct ShardHits {
    std::vector<uint32_t> docs, freqs;
    std::vector<float> scores;
    std::vector<uint64_t> off;
    bool ran = false;
  };
  const size_t G = n->shards.size();
  std::vector<ShardHits> sh(G);
  // one shard's batch: once with a guessed payload size, once more with the size it reports
  if (int rc = n->pool->run([&](uint32_t g) {
        tfidf_index *ix = n->shards[g];
        ShardHits &b = sh[g];
        if (!index_committed(ix) || index_num_docs(ix) == 0) return (int)TFIDF_OK;
        b.off.assign((size_t)n_p + 1, 0);
        uint64_t total = 0, guess = std::min<uint64_t>(64ull * n_p + 4096, 1ull << 24);
        int rc = TFIDF_OK;
        for (int attempt = 0; attempt < 2; attempt++) {
          b.docs.resize(guess);
          b.scores.resize(guess);
          b.freqs.resize(guess);
          rc = sloppy ? tfidf_search_phrase_slop_batch(ix, p_utf8, p_offsets, slops, n_p, b.docs.data(),
                                                       b.scores.data(), reinterpret_cast<float *>(b.freqs.data()),
                                                       guess, b.off.data(), &total)
                      : tfidf_search_phrase_batch(ix, p_utf8, p_offsets, n_p, b.docs.data(), b.scores.data(),
                                                  b.freqs.data(), guess, b.off.data(), &total);
          if (rc != TFIDF_E_BUFFER) break;
          guess = total;
        }
        b.ran = rc == TFIDF_OK;
        return rc;
      }))
    return rc;
  uint64_t total = 0;
  hit_offsets[0] = 0;
  for (uint32_t i = 0; i < n_p; i++) {
    for (size_t g = 0; g < G; g++)
      if (sh[g].ran) total += sh[g].off[i + 1] - sh[g].off[i];
    hit_offsets[i + 1] = total;
  }
  *n_out = total;
  if (total > cap) return errf(TFIDF_E_BUFFER, "need %llu result slots", (unsigned long long)total);
  // the shards' lists of a phrase are ordered, and ascending shard = ascending global id among equal scores
  std::vector<uint64_t> at(G);
  for (uint32_t i = 0; i < n_p; i++) {
    for (size_t g = 0; g < G; g++) at[g] = sh[g].ran ? sh[g].off[i] : 0;
    for (uint64_t o = hit_offsets[i]; o < hit_offsets[i + 1]; o++) {
      size_t best = G;
      for (size_t g = 0; g < G; g++) {
        if (!sh[g].ran || at[g] >= sh[g].off[i + 1]) continue;
        if (best == G || sh[g].scores[at[g]] > sh[best].scores[at[best]]) best = g;
      }
      const uint64_t j = at[best]++;
      doc_ids[o] = n->doc_base[best] + sh[best].docs[j];
      scores[o] = sh[best].scores[j];
      freqs[o] = sh[best].freqs[j];
    }
  }
  return TFIDF_OK;
}

extern "C" int tfidf_node_search_phrase_batch(tfidf_node *n, const uint8_t *p_utf8, const uint64_t *p_offsets,
                                              uint32_t n_p, uint64_t *doc_ids, float *scores, uint32_t *freqs,
                                              uint64_t cap, uint64_t *hit_offsets, uint64_t *n_out) {
  return node_phrase_batch(n, p_utf8, p_offsets, nullptr, false, n_p, doc_ids, scores, freqs, cap, hit_offsets, n_out);
}

extern "C" int tfidf_node_search_phrase_slop_batch(tfidf_node *n, const uint8_t *p_utf8, const uint64_t *p_offsets,
                                                   const uint32_t *slops, uint32_t n_p, uint64_t *doc_ids,
                                                   float *scores, float *freqs, uint64_t cap, uint64_t *hit_offsets,
                                                   uint64_t *n_out) {
  return node_phrase_batch(n, p_utf8, p_offsets, slops, true, n_p, doc_ids, scores,
                           reinterpret_cast<uint32_t *>(freqs), cap, hit_offsets, n_out);
}

// ---------------------------------------------------------------------------
// compound queries over the node: every shard with documents runs the whole
// batch (tfidf_search_compound_batch: its clause routes on the shard's own
// vocabulary and the statistics in force); the host merges each query's ordered
// lists by (score bits descending, global id ascending).

// the validated batch on every shard and the merge; batch(ix, docs, scores, cap, hit_offsets, n_out, ms) is the
// shard's call, what names it in the error before the first commit
template <class Batch>
static int node_compound_run(tfidf_node *n, const char *what, Batch batch, uint32_t n_q, uint64_t *doc_ids,
                             float *scores, uint64_t cap, uint64_t *hit_offsets, uint64_t *n_out, float *ms_device) {
  std::lock_guard<std::mutex> lk(n->mu);
  if (!n->committed) return errf(TFIDF_E_STATE, "%s search before tfidf_node_commit", what);
  struct ShardHits {
    std::vector<uint32_t> docs;
    std::vector<float> scores;
    std::vector<uint64_t> off;
    float ms = 0.0f;
    bool ran = false;
  };
  const size_t G = n->shards.size();
  std::vector<ShardHits> sh(G);
  // one shard's batch: once with a guessed payload size, once more with the size it reports
  if (int rc = n->pool->run([&](uint32_t g) {
        tfidf_index *ix = n->shards[g];
        ShardHits &b = sh[g];
        if (!index_committed(ix) || index_num_docs(ix) == 0) return (int)TFIDF_OK;
        b.off.assign((size_t)n_q + 1, 0);
        uint64_t total = 0, guess = std::min<uint64_t>(64ull * n_q + 4096, 1ull << 24);
        int rc = TFIDF_OK;
        for (int attempt = 0; attempt < 2; attempt++) {
          b.docs.resize(guess);
          b.scores.resize(guess);
          rc = batch(ix, b.docs.data(), b.scores.data(), guess, b.off.data(), &total, &b.ms);
          if (rc != TFIDF_E_BUFFER) break;
          guess = total;
        }
        b.ran = rc == TFIDF_OK;
        return rc;
      }))
    return rc;
  if (ms_device) {
    *ms_device = 0.0f;
    for (size_t g = 0; g < G; g++)
      if (sh[g].ran) *ms_device = std::max(*ms_device, sh[g].ms);   // the shards run at once: the slowest one's time
  }
  uint64_t total = 0;
  hit_offsets[0] = 0;
  for (uint32_t i = 0; i < n_q; i++) {
    for (size_t g = 0; g < G; g++)
      if (sh[g].ran) total += sh[g].off[i + 1] - sh[g].off[i];
    hit_offsets[i + 1] = total;
  }
  *n_out = total;
  if (total > cap) return errf(TFIDF_E_BUFFER, "need %llu result slots", (unsigned long long)total);
  // the shards' lists of a query are ordered, and ascending shard = ascending global id among equal scores
  auto bits = [](float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
  };
  std::vector<uint64_t> at(G);
  for (uint32_t i = 0; i < n_q; i++) {
    for (size_t g = 0; g < G; g++) at[g] = sh[g].ran ? sh[g].off[i] : 0;
    for (uint64_t o = hit_offsets[i]; o < hit_offsets[i + 1]; o++) {
      size_t best = G;
      for (size_t g = 0; g < G; g++) {
        if (!sh[g].ran || at[g] >= sh[g].off[i + 1]) continue;
        if (best == G || bits(sh[g].scores[at[g]]) > bits(sh[best].scores[at[best]])) best = g;
      }
      const uint64_t j = at[best]++;
      doc_ids[o] = n->doc_base[best] + sh[best].docs[j];
      scores[o] = sh[best].scores[j];
    }
  }
  return TFIDF_OK;
}

extern "C" int tfidf_node_search_compound_batch(tfidf_node *n, const uint8_t *c_utf8, const uint64_t *c_offsets,
                                                const tfidf_clause *clauses, const uint64_t *q_clause_offsets,
                                                uint32_t n_q, uint64_t *doc_ids, float *scores, uint64_t cap,
                                                uint64_t *hit_offsets, uint64_t *n_out, float *ms_device) {
  if (!n || !hit_offsets || !n_out || (n_q && !q_clause_offsets) || (cap && (!doc_ids || !scores)))
    return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  if (n_q && n_q <= kCqMaxQueries && q_clause_offsets[n_q] && (!clauses || !c_offsets))
    return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  uint64_t bad = 0;
  if (const int why = cq_check_args(c_offsets, clauses, q_clause_offsets, n_q, &bad))
    return errf(TFIDF_E_INVALID_ARG, "compound arguments: rule %d broken at %llu (compound_plan.h)", why,
                (unsigned long long)bad);
  return node_compound_run(
      n, "compound",
      [&](tfidf_index *ix, uint32_t *d, float *sc, uint64_t room, uint64_t *off, uint64_t *total, float *ms) {
        return tfidf_search_compound_batch(ix, c_utf8, c_offsets, clauses, q_clause_offsets, n_q, d, sc, room, off,
                                           total, ms);
      },
      n_q, doc_ids, scores, cap, hit_offsets, n_out, ms_device);
}

// nested compound queries over the node: the same fan-out and merge over tfidf_search_nested_batch
extern "C" int tfidf_node_search_nested_batch(tfidf_node *n, const uint8_t *c_utf8, const uint64_t *c_offsets,
                                              const tfidf_qnode *nodes, const uint64_t *q_node_offsets, uint32_t n_q,
                                              uint64_t *doc_ids, float *scores, uint64_t cap, uint64_t *hit_offsets,
                                              uint64_t *n_out, float *ms_device) {
  if (!n || !hit_offsets || !n_out || (n_q && !q_node_offsets) || (cap && (!doc_ids || !scores)))
    return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  if (n_q && n_q <= kCqMaxQueries && q_node_offsets[n_q] && (!nodes || !c_offsets))
    return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  uint64_t bad_q = 0, bad_n = 0;
  if (const int why = cqn_check_args(c_offsets, nodes, q_node_offsets, n_q, &bad_q, &bad_n))
    return errf(TFIDF_E_INVALID_ARG, "nested arguments: rule %d broken at query %llu node %llu (compound_tree_plan.h)",
                why, (unsigned long long)bad_q, (unsigned long long)bad_n);
  return node_compound_run(
      n, "nested",
      [&](tfidf_index *ix, uint32_t *d, float *sc, uint64_t room, uint64_t *off, uint64_t *total, float *ms) {
        return tfidf_search_nested_batch(ix, c_utf8, c_offsets, nodes, q_node_offsets, n_q, d, sc, room, off, total,
                                         ms);
      },
      n_q, doc_ids, scores, cap, hit_offsets, n_out, ms_device);
}

// ---------------------------------------------------------------------------
// fuzzy search over the node: every shard with documents expands each term over
// its own vocabulary and scores it under the statistics in force
// (tfidf_search_fuzzy_batch); the host merges each term's lists as the phrase
// search merges them.

extern "C" int tfidf_node_search_fuzzy_batch(tfidf_node *n, const uint8_t *t_utf8, const uint64_t *t_offsets,
                                             uint32_t n_terms, uint32_t max_edits, uint32_t prefix_len,
                                             uint32_t max_expansions, uint64_t *doc_ids, float *scores, uint64_t cap,
                                             uint64_t *hit_offsets, uint32_t *n_expanded, uint64_t *n_out,
                                             float *ms_device) {
  if (!n || !hit_offsets || !n_out || (n_terms && (!t_offsets || !n_expanded || (!t_utf8 && t_offsets[n_terms]))) ||
      (cap && (!doc_ids || !scores)))
    return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  if (max_edits > 2) return errf(TFIDF_E_INVALID_ARG, "max_edits %u above 2", max_edits);
  if (max_expansions < 1 || max_expansions > 64)
    return errf(TFIDF_E_INVALID_ARG, "max_expansions %u outside 1..64", max_expansions);
  std::lock_guard<std::mutex> lk(n->mu);
  if (ms_device) *ms_device = 0.0f;
  if (!n->committed) return errf(TFIDF_E_STATE, "fuzzy search before tfidf_node_commit");
  struct ShardHits {
    std::vector<uint32_t> docs, n_exp;
    std::vector<float> scores;
    std::vector<uint64_t> off;
    float ms = 0.0f;
    bool ran = false;
  };
  const size_t G = n->shards.size();
  std::vector<ShardHits> sh(G);
  // one shard's batch: once with a guessed payload size, once more with the size it reports
  if (int rc = n->pool->run([&](uint32_t g) {
        tfidf_index *ix = n->shards[g];
        ShardHits &b = sh[g];
        if (!index_committed(ix) || index_num_docs(ix) == 0) return (int)TFIDF_OK;
        b.off.assign((size_t)n_terms + 1, 0);
        b.n_exp.assign((size_t)n_terms + 1, 0);
        uint64_t total = 0, guess = std::min<uint64_t>(64ull * n_terms + 4096, 1ull << 24);
        int rc = TFIDF_OK;
        for (int attempt = 0; attempt < 2; attempt++) {
          b.docs.resize(guess);
          b.scores.resize(guess);
          rc = tfidf_search_fuzzy_batch(ix, t_utf8, t_offsets, n_terms, max_edits, prefix_len, max_expansions,
                                        b.docs.data(), b.scores.data(), guess, b.off.data(), b.n_exp.data(), &total,
                                        &b.ms);
          if (rc != TFIDF_E_BUFFER) break;
          guess = total;
        }
        b.ran = rc == TFIDF_OK;
        return rc;
      }))
    return rc;
  uint64_t total = 0;
  hit_offsets[0] = 0;
  for (uint32_t i = 0; i < n_terms; i++) {
    n_expanded[i] = 0;
    for (size_t g = 0; g < G; g++)
      if (sh[g].ran) {
        total += sh[g].off[i + 1] - sh[g].off[i];
        n_expanded[i] += sh[g].n_exp[i];
      }
    hit_offsets[i + 1] = total;
  }
  *n_out = total;
  if (ms_device)
    for (const ShardHits &b : sh) *ms_device = std::max(*ms_device, b.ms);
  if (total > cap) return errf(TFIDF_E_BUFFER, "need %llu result slots", (unsigned long long)total);
  // the shards' lists of a term are ordered, and ascending shard = ascending global id among equal scores
  std::vector<uint64_t> at(G);
  for (uint32_t i = 0; i < n_terms; i++) {
    for (size_t g = 0; g < G; g++) at[g] = sh[g].ran ? sh[g].off[i] : 0;
    for (uint64_t o = hit_offsets[i]; o < hit_offsets[i + 1]; o++) {
      size_t best = G;
      for (size_t g = 0; g < G; g++) {
        if (!sh[g].ran || at[g] >= sh[g].off[i + 1]) continue;
        if (best == G || sh[g].scores[at[g]] > sh[best].scores[at[best]]) best = g;
      }
      const uint64_t j = at[best]++;
      doc_ids[o] = n->doc_base[best] + sh[best].docs[j];
      scores[o] = sh[best].scores[j];
    }
  }
  return TFIDF_OK;
}

// ---------------------------------------------------------------------------
// more-like-this over the node: the owning shard selects a seed's terms, every
// shard with documents scores the term strings on its own dictionary and
// statistics, the host merges per seed by (score descending, global id ascending)

extern "C" int tfidf_node_more_like_this_batch(tfidf_node *n, const uint64_t *seeds, uint32_t n_seeds,
                                               const tfidf_mlt_params *params, uint32_t k, uint32_t flags,
                                               uint64_t *doc_ids, float *scores, uint32_t *counts) {
  if (!n || (n_seeds && (!seeds || !doc_ids || !scores || !counts))) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  tfidf_mlt_params p;
  tfidf_mlt_params_init(&p);
  if (params) p = *params;
  if (p.max_terms < 1 || p.max_terms > kMltMaxTerms)
    return errf(TFIDF_E_INVALID_ARG, "max_terms %u outside 1..%u", p.max_terms, kMltMaxTerms);
  const MltRules R{p.min_tf ? p.min_tf : 1u, p.min_df, p.max_df, p.max_terms};
  const bool excl = (flags & TFIDF_MLT_EXCLUDE_SEED) != 0;
  if (flags & ~TFIDF_MLT_EXCLUDE_SEED) return errf(TFIDF_E_INVALID_ARG, "unknown flags 0x%x", flags);
  if (k == 0 || k > (excl ? 1023u : 1024u))
    return errf(TFIDF_E_INVALID_ARG, "more-like-this needs 1 <= k <= %u", excl ? 1023u : 1024u);
  if (n_seeds > kMltMaxSeeds) return errf(TFIDF_E_INVALID_ARG, "more than %u seeds in one call", kMltMaxSeeds);
  std::lock_guard<std::mutex> lk(n->mu);
  if (!n->committed) return errf(TFIDF_E_STATE, "more-like-this before tfidf_node_commit");
  for (uint32_t i = 0; i < n_seeds; i++)
    if (seeds[i] >= n->num_docs)
      return errf(TFIDF_E_INVALID_ARG, "seed %u (doc %llu) out of range: %llu documents", i,
                  (unsigned long long)seeds[i], (unsigned long long)n->num_docs);
  const size_t G = n->shards.size();
  // seeds to their shards (tfidf_node_doc_key's rule)
  struct Owned {
    std::vector<uint32_t> local, at;
    MltLists ml;
  };
  std::vector<Owned> own(G);
  for (uint32_t i = 0; i < n_seeds; i++) {
    size_t g = G - 1;
    while (n->doc_base[g] > seeds[i]) g--;
    own[g].local.push_back((uint32_t)(seeds[i] - n->doc_base[g]));
    own[g].at.push_back(i);
  }
  if (int rc = n->pool->run([&](uint32_t g) {
        if (own[g].local.empty()) return (int)TFIDF_OK;
        return index_mlt_terms(n->shards[g], own[g].local.data(), (uint32_t)own[g].local.size(), R, &own[g].ml);
      }))
    return rc;
  std::vector<std::vector<std::string>> lists(n_seeds);
  for (size_t g = 0; g < G; g++)
    for (size_t j = 0; j < own[g].at.size(); j++)
      for (const MltTerm &t : own[g].ml.terms[j]) lists[own[g].at[j]].push_back(t.term);
  const uint32_t kk = excl ? k + 1 : k;
  struct ShardTop {
    std::vector<uint32_t> docs, cnt;
    std::vector<float> scores;
    bool ran = false;
  };
  std::vector<ShardTop> sh(G);
  if (int rc = n->pool->run([&](uint32_t g) {
        tfidf_index *ix = n->shards[g];
        if (n_seeds == 0 || !index_committed(ix) || index_num_docs(ix) == 0) return (int)TFIDF_OK;
        ShardTop &b = sh[g];
        b.docs.resize((size_t)n_seeds * kk);
        b.scores.resize((size_t)n_seeds * kk);
        b.cnt.assign(n_seeds, 0);
        const int rc = index_search_term_lists(ix, lists, kk, b.docs.data(), b.scores.data(), b.cnt.data());
        b.ran = rc == TFIDF_OK;
        return rc;
      }))
    return rc;
  struct Hit {
    float score;
    uint64_t doc;
  };
  std::vector<Hit> all;
  for (uint32_t i = 0; i < n_seeds; i++) {
    all.clear();
    for (size_t g = 0; g < G; g++) {
      if (!sh[g].ran) continue;
      for (uint32_t j = 0; j < sh[g].cnt[i]; j++) {
        const uint64_t d = n->doc_base[g] + sh[g].docs[(size_t)i * kk + j];
        if (excl && d == seeds[i]) continue;
        all.push_back(Hit{sh[g].scores[(size_t)i * kk + j], d});
      }
    }
    std::sort(all.begin(), all.end(), [](const Hit &x, const Hit &y) {
      if (x.score != y.score) return x.score > y.score;
      return x.doc < y.doc;
    });
    const uint32_t m = (uint32_t)std::min<size_t>(k, all.size());
    for (uint32_t j = 0; j < m; j++) {
      doc_ids[(size_t)i * k + j] = all[j].doc;
      scores[(size_t)i * k + j] = all[j].score;
    }
    counts[i] = m;
  }
  return TFIDF_OK;
}

extern "C" int tfidf_node_stats_get(const tfidf_node *n, tfidf_node_stats *out) {
  if (!n || !out) return errf(TFIDF_E_INVALID_ARG, "NULL argument");
  out->n_shards = n->shards.size();
  out->num_docs = n->num_docs;
  out->doc_count = n->doc_count;
  out->sum_ttf = n->sum_ttf;
  out->num_terms = n->num_terms;
  out->transport = (uint64_t)n->transport;
  return TFIDF_OK;
}
