// C ABI of the MI355X Reed-Solomon path (include/callfs_rs.h): the context and what every
// call shares -- device selection and lanes, the coefficient tables and their device
// layout, rs_host_alloc memory, the host-side matrices -- and batched SHA-256.
//
// Host side of the drop-in for erasure/codec.go. The host-memory entry points are in
// rs_host.cpp, the device-resident plans in rs_plan.cpp; every byte of GF(2^8) arithmetic
// over shard data runs in the HIP kernels of rs_kernels.hip and rs_mixed.hip.
#include "rs_internal.hpp"
#include "sha256.hpp"

using namespace callfs;

namespace callfs {

// ---- coefficient tables -----------------------------------------------------------

namespace {

// verify=false drops the check rows (plain Reconstruct); wanted as for decode_plan.
std::shared_ptr<const Tables> build_tables(int k, int m, const uint8_t* present, bool verify,
                                           const uint8_t* wanted) {
  DecodePlan dp;
  if (!decode_plan(k, m, present, wanted, dp)) return nullptr;
  auto t = std::make_shared<Tables>();
  t->k = k;
  t->m = m;
  t->valid = dp.valid;
  t->missing = dp.missing;
  if (verify) t->check = dp.check;
  const int nrows = static_cast<int>(t->missing.size() + t->check.size());
  for (int g0 = 0; g0 < nrows; g0 += kMaxRowsPerLaunch) {
    Group g;
    const int R = std::min(kMaxRowsPerLaunch, nrows - g0);
    g.tabs.assign(static_cast<size_t>(k) * R * kTabWords, 0);
    for (int r = 0; r < R; ++r) {
      const int row = g0 + r;
      const bool is_check = row >= static_cast<int>(t->missing.size());
      g.shard.push_back(is_check ? t->check[row - t->missing.size()] : t->missing[row]);
      if (is_check) g.verify_mask |= 1u << r;
      for (int i = 0; i < k; ++i)
        perm_tables(dp.rows.at(row, i), &g.tabs[(static_cast<size_t>(i) * R + r) * kTabWords]);
    }
    const size_t per_shard = 32u * nibble_width(R);
    g.ltabs.assign(static_cast<size_t>(k) * per_shard, 0);
    for (int i = 0; i < k; ++i) {
      uint8_t col[kMaxRowsPerLaunch] = {0};
      for (int r = 0; r < R; ++r) col[r] = dp.rows.at(g0 + r, i);
      nibble_tables(col, R, &g.ltabs[static_cast<size_t>(i) * per_shard]);
    }
    if (R >= kBitsliceMinRows && bs::mode() != bs::Mode::kOff) {
      std::vector<uint8_t> coef(static_cast<size_t>(R) * k);
      for (int r = 0; r < R; ++r)
        for (int i = 0; i < k; ++i) coef[static_cast<size_t>(r) * k + i] = dp.rows.at(g0 + r, i);
      g.bsk = bs::kernel_for(k, R, coef.data());
    }
    t->groups.push_back(std::move(g));
  }
  return t;
}

}  // namespace

std::shared_ptr<const Tables> TableCache::get(int k, int m, const uint8_t* present, bool verify,
                                              const uint8_t* wanted) {
  std::string key;
  key.reserve(k + m + 8);
  key.append(reinterpret_cast<const char*>(&k), sizeof k);
  key.append(reinterpret_cast<const char*>(&m), sizeof m);
  key.push_back(verify ? 'v' : 'r');
  // '0' a missing shard that is rebuilt, 'u' one nobody wants: all wanted = the key of null
  for (int i = 0; i < k + m; ++i)
    key.push_back(present[i] ? '1' : (!wanted || wanted[i]) ? '0' : 'u');
  {
    std::lock_guard<std::mutex> g(mu_);
    auto it = map_.find(key);
    if (it != map_.end()) return it->second;
  }
  auto t = build_tables(k, m, present, verify, wanted);
  if (!t) return nullptr;
  std::lock_guard<std::mutex> g(mu_);
  if (map_.size() >= kCap) map_.clear();
  map_.emplace(key, t);
  return t;
}

MetaLayout meta_layout(const Tables& t, int batch) {
  MetaLayout L;
  Packer pk;
  L.status_off = pk.take(sizeof(int) * static_cast<size_t>(batch));
  L.in_off = pk.take(sizeof(void*) * static_cast<size_t>(batch) * t.k);
  for (const Group& g : t.groups) {
    L.out_off.push_back(pk.take(sizeof(void*) * static_cast<size_t>(batch) * g.shard.size()));
    L.tab_off.push_back(pk.take(sizeof(uint32_t) * g.tabs.size()));
    L.ltab_off.push_back(pk.take(g.ltabs.size()));
  }
  L.total = pk.off;
  return L;
}

ApplyArgs group_args(const Tables& t, const MetaLayout& L, size_t gi, int batch, uint8_t* d,
                     size_t S, int status_stride, const LayoutHint& hint) {
  const Group& g = t.groups[gi];
  ApplyArgs a{};
  a.in_tab = reinterpret_cast<const uint8_t* const*>(d + L.in_off);
  a.out_tab = reinterpret_cast<uint8_t* const*>(d + L.out_off[gi]);
  a.tabs = reinterpret_cast<const uint32_t*>(d + L.tab_off[gi]);
  a.ltabs = d + L.ltab_off[gi];
  a.S = S;
  a.verify_mask = g.verify_mask;
  a.status = reinterpret_cast<int*>(d + L.status_off);
  a.status_stride = status_stride;
  a.K = t.k;
  a.R = static_cast<int>(g.shard.size());
  a.batch = batch;
  a.addr_tz = hint.addr_tz;
  a.stripe_stride = hint.stripe_stride;
  a.in_misalign = hint.in_misalign;
  a.out_misalign = hint.out_misalign;
  a.bs = g.bsk.get();
  return a;
}

hipError_t launch_groups(const Tables& t, const MetaLayout& L, int batch, uint8_t* d, size_t S,
                         hipStream_t s, int status_stride, const LayoutHint& hint,
                         const std::vector<int>* orders, LaunchEvents ev) {
  const size_t ng = t.groups.size();
  for (size_t gi = 0; gi < ng; ++gi) {
    const ApplyArgs a = group_args(t, L, gi, batch, d, S, status_stride, hint);
    // a plan's pinned or tuned order; else what rs_plan_tune measured for this shape on the
    // device (tune_table.hpp); else the rule
    int order = orders && gi < orders->size() ? (*orders)[gi] : -1;
    if (order < 0) order = tuned_order(a);
    hipError_t e = launch_apply(a, s, /*bytes_only=*/false, order, group_events(ev, gi, ng));
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace callfs

// ---- context ------------------------------------------------------------------------

// CALLFS_RS_HOST_POOL_BYTES: the cap on parked rs_host_alloc bytes (host_path.hpp HostPool)
static size_t host_pool_limit() {
  static const size_t v = [] {
    const char* e = std::getenv("CALLFS_RS_HOST_POOL_BYTES");
    return e ? static_cast<size_t>(std::strtoull(e, nullptr, 0)) : (4ull << 30);
  }();
  return v;
}

rs_ctx::rs_ctx() : host_pool(host_pool_limit()) {}

rs_ctx::~rs_ctx() {
  for (void* p : pinned.all()) (void)hipHostFree(p);  // buffers the caller did not free
  for (void* p : host_pool.drain()) (void)hipHostFree(p);
  for (auto& d : devs) {
    (void)hipSetDevice(d->id);
    for (auto& l : d->lanes) {
      for (Slot& sl : l->slot) {
        if (sl.stream) (void)hipStreamSynchronize(sl.stream);
        sl.dev.release();
        sl.host.release();
        sl.meta.release();
        sl.hmeta.release();
        sl.hstat.release();
        sl.small.release();
        sl.small_tabs.release();
        sl.small_counter.release();
        if (sl.done) (void)hipEventDestroy(sl.done);
        if (sl.stream) (void)hipStreamDestroy(sl.stream);
      }
    }
  }
}

Device* rs_ctx::device(int id) {
  for (auto& d : devs)
    if (d->id == id) return d.get();
  return nullptr;
}

Lane* rs_ctx::acquire(Device* d) {
  std::unique_lock<std::mutex> g(d->mu);
  for (;;) {
    if (!d->free_lanes.empty()) {
      Lane* l = d->free_lanes.back();
      d->free_lanes.pop_back();
      return l;
    }
    if (static_cast<int>(d->lanes.size()) < kMaxLanesPerDevice) {
      auto l = std::make_unique<Lane>();
      if (hipSetDevice(d->id) != hipSuccess) return nullptr;
      for (Slot& sl : l->slot)
        if (hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&sl.done, hipEventDisableTiming) != hipSuccess) {
          for (Slot& s : l->slot) {  // a partly built lane is not kept: free what exists
            if (s.done) (void)hipEventDestroy(s.done);
            if (s.stream) (void)hipStreamDestroy(s.stream);
          }
          return nullptr;
        }
      d->lanes.push_back(std::move(l));
      return d->lanes.back().get();
    }
    d->cv.wait(g);
  }
}

void rs_ctx::release(Device* d, Lane* l) {
  {
    std::lock_guard<std::mutex> g(d->mu);
    d->free_lanes.push_back(l);
  }
  d->cv.notify_one();
}

// ---- exported -------------------------------------------------------------------------

extern "C" {

int rs_abi_version(void) { return RS_ABI_VERSION; }

const char* rs_strerror(int code) {
  switch (code) {
    case RS_OK: return "ok";
    case RS_E_INVALID_PROFILE: return "erasure: invalid erasure profile parameters (code 3054)";
    case RS_E_SHORT_DATA: return "not enough data to fill the number of requested shards";
    case RS_E_TOO_FEW_SHARDS: return "too few shards given";
    case RS_E_SHARD_SIZE: return "shard sizes do not match";
    case RS_E_NO_DATA: return "no shard data";
    case RS_E_CORRUPT: return "erasure: shard checksum mismatch (code 3051)";
    case RS_E_INSUFFICIENT: return "erasure: insufficient shards for reconstruction (code 3050)";
    case RS_E_UNSUPPORTED: return "profile needs the GF(2^16) (Leopard) codec: k+m > 256";
    case RS_E_HIP: return "HIP runtime error or no usable device";
    case RS_E_ARG: return "invalid argument";
    case RS_E_SINGULAR: return "matrix is singular";
    case RS_E_NOMEM: return "out of memory";
    default: return "unknown error";
  }
}

int rs_init(rs_ctx** out, unsigned device_mask) {
  if (!out) return RS_E_ARG;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return RS_E_HIP;
  auto ctx = std::make_unique<rs_ctx>();
  for (int d : select_devices(count, device_mask)) {
    auto dev = std::make_unique<Device>();
    dev->id = d;
    ctx->devs.push_back(std::move(dev));
  }
  if (ctx->devs.empty()) return RS_E_HIP;
  // (the wide kernels' > 64 KiB dynamic-LDS opt-in is a per-device attribute: launch_apply
  // issues it once per (device, R) before the first such launch on a device, so rs_init
  // touches no device -- a process per GPU must not load code onto all eight)
  *out = ctx.release();
  return RS_OK;
}

void rs_shutdown(rs_ctx* ctx) {
  DeviceGuard dg;
  delete ctx;
}

int rs_device_count(const rs_ctx* ctx) { return ctx ? static_cast<int>(ctx->devs.size()) : 0; }

int rs_host_alloc(rs_ctx* ctx, size_t bytes, void** out) {
  if (!ctx || !out || bytes == 0) return RS_E_ARG;
  *out = nullptr;
  HostPool::Buf b = ctx->host_pool.take(bytes);
  if (!b.p) {
    b.cap = HostPool::granule(bytes);
    // portable: every device of the context may use it. Coherent: the kernels read and
    // write it in place (zero-copy), and the caller refills the same buffer between
    // calls, so device caches must not keep its lines across launches.
    if (hipHostMalloc(&b.p, b.cap, hipHostMallocPortable | hipHostMallocCoherent) != hipSuccess)
      return RS_E_NOMEM;
  }
  ctx->pinned.add(b.p, b.cap);
  *out = b.p;
  return RS_OK;
}

int rs_host_free(rs_ctx* ctx, void* p) {
  if (!ctx || !p) return RS_E_ARG;
  const size_t cap = ctx->pinned.size_of(p);
  if (!cap || !ctx->pinned.remove(p)) return RS_E_ARG;
  int rc = RS_OK;
  for (void* q : ctx->host_pool.put(p, cap))
    if (hipHostFree(q) != hipSuccess) rc = RS_E_HIP;
  return rc;
}

int rs_host_counters_read(const rs_ctx* ctx, rs_host_counters* out) {
  if (!ctx || !out) return RS_E_ARG;
  out->calls = ctx->n_calls.load(std::memory_order_relaxed);
  out->chunks = ctx->n_chunks.load(std::memory_order_relaxed);
  out->launches = ctx->n_launches.load(std::memory_order_relaxed);
  out->copies = ctx->n_copies.load(std::memory_order_relaxed);
  out->ragged_calls = ctx->n_ragged_calls.load(std::memory_order_relaxed);
  return RS_OK;
}

int rs_shard_size(int k, int m, int64_t len, int64_t* shard_size) {
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!shard_size || len < 0) return RS_E_ARG;
  if (len == 0) return RS_E_SHORT_DATA;
  *shard_size = (len + k - 1) / k;
  return RS_OK;
}

int rs_encode_matrix(int k, int m, uint8_t* out) {
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!out) return RS_E_ARG;
  Mat E;
  if (!encode_matrix(k, m, E)) return RS_E_SINGULAR;
  std::memcpy(out, E.v.data(), E.v.size());
  return RS_OK;
}

int rs_decode_rows(int k, int m, const uint8_t* present, int* valid_out, int* missing_out,
                   int* n_missing, uint8_t* rows_out) {
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!present || !valid_out || !missing_out || !n_missing || !rows_out) return RS_E_ARG;
  int np = 0;
  for (int i = 0; i < k + m; ++i) np += present[i] != 0;
  if (np < k) return RS_E_TOO_FEW_SHARDS;
  DecodePlan dp;
  if (!decode_plan(k, m, present, dp)) return RS_E_SINGULAR;
  std::copy(dp.valid.begin(), dp.valid.end(), valid_out);
  std::copy(dp.missing.begin(), dp.missing.end(), missing_out);
  *n_missing = static_cast<int>(dp.missing.size());
  std::memcpy(rows_out, dp.rows.v.data(), dp.missing.size() * static_cast<size_t>(k));
  return RS_OK;
}

// ---- batched SHA-256 (ShardChecksum) ------------------------------------------------

struct rs_hash_plan {
  int device = 0;
  int count = 0;
  int mpw = 1;
  DevBuf dtab;  // [count] pointers then [count] lengths
  ~rs_hash_plan() {
    if (dtab.p) (void)hipSetDevice(device);  // the buffer is freed on the plan's device
  }
};

int rs_sha256_plan_create(rs_ctx* ctx, int device, const uint8_t* const* msgs,
                          const uint64_t* lens, int count, rs_hash_plan** out) {
  DeviceGuard dg;
  if (!ctx || !out || count < 0 || (count && (!msgs || !lens))) return RS_E_ARG;
  *out = nullptr;
  if (!ctx->device(device)) return RS_E_ARG;
  auto plan = std::make_unique<rs_hash_plan>();
  plan->device = device;
  plan->count = count;
  plan->mpw = default_msgs_per_wave(count);
  if (const char* e = kAbInstances ? std::getenv("CALLFS_SHA_MSGS_PER_WAVE") : nullptr)
    plan->mpw = std::atoi(e);
  HIPCHK(hipSetDevice(device));
  if (count) {
    std::vector<uint8_t> h(static_cast<size_t>(count) * (sizeof(void*) + sizeof(uint64_t)));
    std::memcpy(h.data(), msgs, count * sizeof(void*));
    std::memcpy(h.data() + count * sizeof(void*), lens, count * sizeof(uint64_t));
    if (const int rc = upload(plan->dtab, device, h.data(), h.size())) return rc;
  }
  *out = plan.release();
  return RS_OK;
}

int rs_sha256_plan_launch(rs_hash_plan* plan, uint8_t* digests, void* stream) {
  DeviceGuard dg;
  if (!plan || (plan->count && !digests)) return RS_E_ARG;
  if ((reinterpret_cast<uintptr_t>(digests) & 3u) != 0) return RS_E_ARG;
  HIPCHK(hipSetDevice(plan->device));
  Sha256Args a{};
  a.msgs = static_cast<const uint8_t* const*>(plan->dtab.p);
  a.lens = reinterpret_cast<const uint64_t*>(static_cast<uint8_t*>(plan->dtab.p) +
                                             plan->count * sizeof(void*));
  a.digests = reinterpret_cast<uint32_t*>(digests);
  a.count = plan->count;
  HIPCHK(launch_sha256(a, plan->mpw, static_cast<hipStream_t>(stream)));
  return RS_OK;
}

void rs_sha256_plan_destroy(rs_hash_plan* plan) {
  DeviceGuard dg;
  delete plan;
}

int rs_sha256_dev(rs_ctx* ctx, int device, const uint8_t* const* msgs, const uint64_t* lens,
                  int count, uint8_t* digests, void* stream) {
  rs_hash_plan* p = nullptr;
  int rc = rs_sha256_plan_create(ctx, device, msgs, lens, count, &p);
  if (rc) return rc;
  rc = rs_sha256_plan_launch(p, digests, stream);
  if (!rc && hipStreamSynchronize(static_cast<hipStream_t>(stream)) != hipSuccess) rc = RS_E_HIP;
  rs_sha256_plan_destroy(p);
  return rc;
}

}  // extern "C"
