// Device-resident plans of the C ABI (include/callfs_rs.h): tables uploaded once for
// repeated, graph-capturable launches over shards in device memory -- uniform plans (one
// erasure pattern, one shard size: every kernel form and tile order), mixed plans (a
// pattern per stripe) and ragged plans (a shard size per stripe too,
// §5.9) and required plans (only the missing shards a caller wants, §5.10) -- the tile-order tuner and the one-shot device calls built on them.
#include <cstdio>

#include "mixed_tables.hpp"
#include "ragged_tables.hpp"
#include "rs_internal.hpp"
#include "tune_table.hpp"

using namespace callfs;

static_assert(kRaggedTileVecs == kRaggedLaunchTileVecs, "the tile map counts the kernel's tiles");

// A mixed plan (rs_plan_create_mixed): the pattern tables and where each piece sits in the
// plan's device buffer.
// A ragged plan (rs_plan_create_ragged) is a mixed plan with a tile map: `ragged` is set,
// the plan's S is the largest shard size (never 0) and each stripe's own size sits in the
// device buffer with tile0 and tile_stripe (ragged_tables.hpp).
// A required plan (rs_plan_create_required) is a ragged plan whose patterns have their own
// row counts: `some` is set, every launch group has its own tile map (g_*) and the patterns'
// row counts inside it (nrows_off).
struct MixedPlan {
  MixedTables t;
  size_t in_off = 0, pat_off = 0;
  std::vector<size_t> out_off, vmask_off, arena_off;  // per launch group
  bool ragged = false;
  bool any_tail = false;  // some stripe's size is no multiple of 16
  uint32_t ntiles = 0;
  size_t size_off = 0, tile0_off = 0, tile_stripe_off = 0;
  bool some = false;
  std::vector<size_t> nrows_off, g_tile0_off, g_tile_stripe_off;  // per launch group
  std::vector<uint32_t> g_ntiles;
  std::vector<uint8_t> g_any_tail;
};

struct rs_plan {
  int device = 0;
  size_t S = 0;
  int batch = 0;
  uint64_t bytes = 0;
  DevBuf dmeta;           // everything a launch reads, and the per-stripe status words
  size_t status_off = 0;  // of the `batch` status words in dmeta
  // A uniform plan: its tables and their layout in dmeta. Its launch groups have tile
  // orders: `orders` holds per group the order from rs_plan_tune / rs_plan_set_orders,
  // -1 = the rule (written by those under `mu`, read by launches).
  std::shared_ptr<const Tables> tables;
  MetaLayout layout;
  LayoutHint hint;
  std::vector<int> orders;
  mutable std::mutex mu;
  // A mixed or ragged plan (`tables` is null): one kernel form in one tile order,
  // `fixed_form`, for every launch group; nothing to tune, pin or bound by a ceiling.
  std::unique_ptr<MixedPlan> mixed;
  int fixed_form = -1;

  bool has_orders() const { return fixed_form < 0; }
  std::vector<int> orders_snapshot() const {
    std::lock_guard<std::mutex> g(mu);
    return orders;
  }
  ~rs_plan() {
    if (dmeta.p) (void)hipSetDevice(device);  // the buffer is freed on the plan's device
  }
};

namespace {

// ---- what differs between uniform, mixed and ragged plans -------------------------------

size_t plan_groups(const rs_plan& plan) {
  return plan.mixed ? plan.mixed->t.groups.size() : plan.tables->groups.size();
}

// The arguments of launch group gi. A mixed or ragged plan's per-stripe tables go to *x
// (the MixedArgs fields, and the tile map of a ragged plan).
ApplyArgs plan_group_args(const rs_plan& plan, size_t gi, RaggedArgs* x = nullptr,
                          const uint32_t** nrows = nullptr) {
  auto* d = static_cast<uint8_t*>(plan.dmeta.p);
  if (!plan.mixed)
    return group_args(*plan.tables, plan.layout, gi, plan.batch, d, plan.S, 1, plan.hint);
  const MixedPlan& mp = *plan.mixed;
  const MixedGroup& g = mp.t.groups[gi];
  ApplyArgs a{};
  a.in_tab = reinterpret_cast<const uint8_t* const*>(d + mp.in_off);
  a.out_tab = reinterpret_cast<uint8_t* const*>(d + mp.out_off[gi]);
  a.ltabs = d + mp.arena_off[gi];
  a.S = plan.S;
  a.status = reinterpret_cast<int*>(d + plan.status_off);
  a.status_stride = 1;
  a.K = mp.t.k;
  a.R = g.R;
  a.batch = plan.batch;
  if (x) {
    x->pat = reinterpret_cast<const uint32_t*>(d + mp.pat_off);
    x->vmask = reinterpret_cast<const uint32_t*>(d + mp.vmask_off[gi]);
    x->tab_stride = static_cast<uint32_t>(g.tab_stride);
    if (mp.ragged) {
      x->size = reinterpret_cast<const uint64_t*>(d + mp.size_off);
      x->tile0 = reinterpret_cast<const uint32_t*>(d + mp.tile0_off);
      x->tile_stripe = reinterpret_cast<const uint32_t*>(d + mp.tile_stripe_off);
      x->ntiles = mp.ntiles;
    }
    if (mp.some) {  // the launch group's own tile map
      x->tile0 = reinterpret_cast<const uint32_t*>(d + mp.g_tile0_off[gi]);
      x->tile_stripe = reinterpret_cast<const uint32_t*>(d + mp.g_tile_stripe_off[gi]);
      x->ntiles = mp.g_ntiles[gi];
      if (nrows) *nrows = reinterpret_cast<const uint32_t*>(d + mp.nrows_off[gi]);
    }
  }
  return a;
}

// Every launch group on stream s; ev as for launch_groups. `orders` counts for plans that
// have tile orders.
hipError_t plan_launch(const rs_plan& plan, hipStream_t s, const std::vector<int>& orders,
                       LaunchEvents ev) {
  if (!plan.mixed)
    return launch_groups(*plan.tables, plan.layout, plan.batch, static_cast<uint8_t*>(plan.dmeta.p),
                         plan.S, s, /*status_stride=*/1, plan.hint, &orders, ev);
  const size_t ng = plan_groups(plan);
  for (size_t gi = 0; gi < ng; ++gi) {
    RaggedArgs r{};
    const uint32_t* nrows = nullptr;
    const ApplyArgs a = plan_group_args(plan, gi, &r, &nrows);
    const LaunchEvents g = group_events(ev, gi, ng);
    const hipError_t e = plan.mixed->some
                             ? launch_ragged_some(a, RaggedSomeArgs{r, nrows},
                                                  plan.mixed->g_any_tail[gi] != 0, s, g)
                         : plan.mixed->ragged
                             ? launch_ragged(a, r, plan.mixed->any_tail, s, g)
                             : launch_mixed(a, MixedArgs{r.pat, r.vmask, r.tab_stride}, s, g);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ---- plan construction --------------------------------------------------------------------

// The common head of the three constructors' argument checks done, a plan on `device`.
std::unique_ptr<rs_plan> new_plan(int device, size_t S, int batch) {
  auto plan = std::make_unique<rs_plan>();
  plan->device = device;
  plan->S = S;
  plan->batch = batch;
  return plan;
}

// Lays out and uploads the device buffer of a mixed plan (plan.mixed->t built, plan.device
// and plan.batch set): the status words, the shard-pointer tables, pat and per launch group
// the compare masks and the table arena, each piece 256-B aligned. With `rg` (a ragged plan)
// also the stripes' sizes, tile0 and tile_stripe. With `rq` (a required plan) the sizes and
// per launch group its tile map and the patterns' row counts; an out_tab slot at or past a
// stripe's row count holds null, and a shard no row names is in no table.
int upload_mixed(rs_plan& plan, uint8_t* const* shards, const RaggedTables* rg,
                 const RequiredTables* rq = nullptr) {
  MixedPlan& mp = *plan.mixed;
  const int k = mp.t.k, n = mp.t.k + mp.t.m, batch = plan.batch;
  Packer pk;
  const size_t P = mp.t.patterns.size();
  plan.status_off = pk.take(sizeof(int) * static_cast<size_t>(batch));
  mp.in_off = pk.take(sizeof(void*) * static_cast<size_t>(batch) * k);
  mp.pat_off = pk.take(sizeof(uint32_t) * static_cast<size_t>(batch));
  for (const MixedGroup& g : mp.t.groups) {
    mp.out_off.push_back(pk.take(sizeof(void*) * static_cast<size_t>(batch) * g.R));
    mp.vmask_off.push_back(pk.take(sizeof(uint32_t) * P));
    mp.arena_off.push_back(pk.take(g.arena.size()));
  }
  if (rg) {
    mp.size_off = pk.take(sizeof(uint64_t) * rg->size.size());
    mp.tile0_off = pk.take(sizeof(uint32_t) * rg->tile0.size());
    mp.tile_stripe_off = pk.take(sizeof(uint32_t) * rg->tile_stripe.size());
  }
  if (rq) {
    mp.size_off = pk.take(sizeof(uint64_t) * rq->size.size());
    for (size_t gi = 0; gi < mp.t.groups.size(); ++gi) {
      const GroupTileMap& gm = rq->maps[gi];
      mp.nrows_off.push_back(pk.take(sizeof(uint32_t) * P));
      mp.g_tile0_off.push_back(pk.take(sizeof(uint32_t) * gm.tile0.size()));
      mp.g_tile_stripe_off.push_back(pk.take(sizeof(uint32_t) * std::max<size_t>(1, gm.tile_stripe.size())));
      mp.g_ntiles.push_back(gm.ntiles);
      mp.g_any_tail.push_back(gm.any_tail);
    }
  }
  std::vector<uint8_t> h(pk.off, 0);
  auto shard_ptr = [&](int b, int i) { return shards[static_cast<size_t>(b) * n + i]; };
  auto* in = reinterpret_cast<const uint8_t**>(h.data() + mp.in_off);
  for (int b = 0; b < batch; ++b) {
    const MixedPattern& pt = mp.t.patterns[mp.t.pat[b]];
    for (int i = 0; i < k; ++i) in[static_cast<size_t>(b) * k + i] = shard_ptr(b, pt.valid[i]);
  }
  std::memcpy(h.data() + mp.pat_off, mp.t.pat.data(), sizeof(uint32_t) * mp.t.pat.size());
  for (size_t gi = 0; gi < mp.t.groups.size(); ++gi) {
    const MixedGroup& g = mp.t.groups[gi];
    auto* o = reinterpret_cast<uint8_t**>(h.data() + mp.out_off[gi]);
    for (int b = 0; b < batch; ++b) {
      const MixedPattern& pt = mp.t.patterns[mp.t.pat[b]];
      for (int r = 0; r < g.R; ++r)
        o[static_cast<size_t>(b) * g.R + r] =
            static_cast<size_t>(g.row0 + r) < pt.rows.size() ? shard_ptr(b, pt.rows[g.row0 + r]) : nullptr;
    }
    std::memcpy(h.data() + mp.vmask_off[gi], g.vmask.data(), sizeof(uint32_t) * P);
    std::memcpy(h.data() + mp.arena_off[gi], g.arena.data(), g.arena.size());
  }
  if (rg) {
    std::memcpy(h.data() + mp.size_off, rg->size.data(), sizeof(uint64_t) * rg->size.size());
    std::memcpy(h.data() + mp.tile0_off, rg->tile0.data(), sizeof(uint32_t) * rg->tile0.size());
    std::memcpy(h.data() + mp.tile_stripe_off, rg->tile_stripe.data(),
                sizeof(uint32_t) * rg->tile_stripe.size());
  }
  if (rq) {
    std::memcpy(h.data() + mp.size_off, rq->size.data(), sizeof(uint64_t) * rq->size.size());
    for (size_t gi = 0; gi < mp.t.groups.size(); ++gi) {
      const GroupTileMap& gm = rq->maps[gi];
      std::memcpy(h.data() + mp.nrows_off[gi], mp.t.groups[gi].nrows.data(), sizeof(uint32_t) * P);
      std::memcpy(h.data() + mp.g_tile0_off[gi], gm.tile0.data(), sizeof(uint32_t) * gm.tile0.size());
      if (!gm.tile_stripe.empty())
        std::memcpy(h.data() + mp.g_tile_stripe_off[gi], gm.tile_stripe.data(),
                    sizeof(uint32_t) * gm.tile_stripe.size());
    }
  }
  if (const int rc = upload(plan.dmeta, plan.device, h.data(), h.size())) return rc;
  // the device copy is all a launch reads: the host arenas can go
  for (MixedGroup& g : mp.t.groups) std::vector<uint8_t>().swap(g.arena);
  return RS_OK;
}

// A timed launch that dispatches no kernel still records both events on the stream, so
// the caller's elapsed time is this launch's (zero), never a stale earlier interval.
int record_empty(void* stream, void* start_event, void* stop_event) {
  const auto s = static_cast<hipStream_t>(stream);
  if (start_event) HIPCHK(hipEventRecord(static_cast<hipEvent_t>(start_event), s));
  if (stop_event) HIPCHK(hipEventRecord(static_cast<hipEvent_t>(stop_event), s));
  return RS_OK;
}

// ---- the tuner's knobs ----------------------------------------------------------------------

constexpr int kTuneRounds = 3;
constexpr float kTuneWarmMs = 150.0f;
constexpr int kTuneWarmBatches = 400;
// CALLFS_RS_TUNE_BAR=<percent>: how much faster than the rule's order another order must
// time to replace it (default 1)
float tune_bar() {
  static const float v = [] {
    const char* e = std::getenv("CALLFS_RS_TUNE_BAR");
    if (e && *e) {
      const float x = std::strtof(e, nullptr);
      if (x >= 0.0f && x < 50.0f) return x;
    }
    return 1.0f;
  }();
  return v;
}

// CALLFS_RS_TUNE_LOG=1: rs_plan_tune prints each candidate's time per launch to stderr
bool tune_log() {
  static const bool on = [] {
    const char* e = std::getenv("CALLFS_RS_TUNE_LOG");
    return e && *e && *e != '0';
  }();
  return on;
}

// The one-shot calls' second half: launch, status, free; RS_E_CORRUPT when a stripe mismatched.
int launch_once(rs_plan* p, void* stream) {
  int rc = rs_plan_launch(p, stream);
  int corrupt = 0;
  if (!rc) rc = rs_plan_status(p, stream, &corrupt);
  rs_plan_destroy(p);
  if (!rc && corrupt) rc = RS_E_CORRUPT;
  return rc;
}

// rs_plan_create's body. wanted (k+m flags, or null: every missing shard): the missing shards
// that get a row; a plan with no row at all has no launch group.
int create_uniform(rs_ctx* ctx, int device, int k, int m, size_t S, int batch,
                   const uint8_t* present, const uint8_t* wanted, uint8_t* const* shards,
                   rs_plan** out);

int one_shot(rs_ctx* ctx, int device, int k, int m, size_t S, int batch, const uint8_t* present,
             uint8_t* const* shards, void* stream) {
  rs_plan* p = nullptr;
  const int rc = rs_plan_create(ctx, device, k, m, S, batch, present, shards, &p);
  if (rc) return rc;
  return launch_once(p, stream);
}

}  // namespace

namespace {

int create_uniform(rs_ctx* ctx, int device, int k, int m, size_t S, int batch,
                   const uint8_t* present, const uint8_t* wanted, uint8_t* const* shards,
                   rs_plan** out) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || !shards || !out || batch < 1) return RS_E_ARG;
  *out = nullptr;
  Device* dev = ctx->device(device);
  if (!dev) return RS_E_ARG;
  const int n = k + m;
  uint8_t pres[256];
  int np = 0;
  for (int i = 0; i < n; ++i) {
    pres[i] = present ? (present[i] != 0) : (i < k);
    np += pres[i];
  }
  if (np < k) return RS_E_TOO_FEW_SHARDS;
  auto t = ctx->cache.get(k, m, pres, true, wanted);
  if (!t) return RS_E_SINGULAR;
  auto plan = new_plan(device, S, batch);
  plan->tables = t;
  plan->layout = meta_layout(*t, batch);
  plan->status_off = plan->layout.status_off;
  // reads: k valid shards + compared parity; writes: missing shards.
  // (a plan with no row reads nothing)
  plan->bytes = t->groups.empty()
                    ? 0
                    : static_cast<uint64_t>(batch) * S * (t->k + t->check.size() + t->missing.size());
  std::vector<uint8_t> h(plan->layout.total);
  plan->hint = fill_meta(*t, plan->layout, batch, h.data(), [&](int b, int i) {
    return static_cast<const uint8_t*>(shards[static_cast<size_t>(b) * n + i]);
  });
  if ((rc = upload(plan->dmeta, device, h.data(), h.size()))) return rc;
  // plans are launched many times: the launch groups the rule gives the bit-sliced kernel have
  // it compiled (or loaded from the code cache) here, so every launch runs it; a compile that
  // fails leaves them on the nibble-table kernels. A plan waits for at most kSyncCompileKR
  // coefficients' worth of compiles (about 4 s on the GPU box); its other blocks compile in
  // the background (RS(200,16) alone: 8 s there, RS(240,16) 48 s on a build host; the 8 groups
  // of an RS(128,128) decode: 30 s) and run the nibble-table kernels until they are ready.
  constexpr int kSyncCompileKR = 2048;
  int sync_kr = 0;
  for (size_t gi = 0; gi < t->groups.size(); ++gi) {
    const Group& g = t->groups[gi];
    if (!g.bsk || !bitslice_wanted(plan_group_args(*plan, gi))) continue;
    const int kr = k * static_cast<int>(g.shard.size());
    const bool wait = sync_kr + kr <= kSyncCompileKR;
    if (wait) sync_kr += kr;
    (void)g.bsk->function(device, wait);
  }
  *out = plan.release();
  return RS_OK;
}

}  // namespace

extern "C" {

// ---- constructors ---------------------------------------------------------------------------

int rs_plan_create(rs_ctx* ctx, int device, int k, int m, size_t S, int batch,
                   const uint8_t* present, uint8_t* const* shards, rs_plan** out) {
  return create_uniform(ctx, device, k, m, S, batch, present, nullptr, shards, out);
}

int rs_plan_create_mixed(rs_ctx* ctx, int device, int k, int m, size_t S, int batch,
                         const uint8_t* present, uint8_t* const* shards, rs_plan** out) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || !shards || !out || !present || batch < 1) return RS_E_ARG;
  *out = nullptr;
  const int n = k + m;
  // every stripe needs k present shards, whichever path the plan takes
  for (int b = 0; b < batch; ++b) {
    int np = 0;
    for (int i = 0; i < n; ++i) np += present[static_cast<size_t>(b) * n + i] != 0;
    if (np < k) return RS_E_TOO_FEW_SHARDS;
  }
  // all masks equal: exactly the uniform plan (its forms, bit-sliced kernels included)
  if (mixed_masks_equal(n, batch, present))
    return rs_plan_create(ctx, device, k, m, S, batch, present, shards, out);
  Device* dev = ctx->device(device);
  if (!dev) return RS_E_ARG;
  auto plan = new_plan(device, S, batch);
  plan->mixed = std::make_unique<MixedPlan>();
  plan->fixed_form = kOrderMixed + RS_ORDER_CONSECUTIVE;
  switch (build_mixed_tables(k, m, batch, present, plan->mixed->t)) {
    case MixedError::kOk: break;
    case MixedError::kTooFewShards: return RS_E_TOO_FEW_SHARDS;
    case MixedError::kSingular: return RS_E_SINGULAR;
    case MixedError::kRowCount: return RS_E_ARG;  // the missing-rows form only
  }
  // reads: k valid shards + the compared shards; writes: the missing ones = n per stripe
  plan->bytes = static_cast<uint64_t>(batch) * S * static_cast<uint64_t>(n);
  rc = upload_mixed(*plan, shards, nullptr);
  if (rc) return rc;
  *out = plan.release();
  return RS_OK;
}

int rs_plan_create_ragged(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                          const uint8_t* present, uint8_t* const* shards, rs_plan** out) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || !sizes || !shards || !out || batch < 1) return RS_E_ARG;
  *out = nullptr;
  const int n = k + m;
  for (int b = 0; b < batch; ++b)
    if (sizes[b] == 0) return RS_E_NO_DATA;  // upstream Encode: ErrShardNoData
  // no masks: every stripe is an encode
  std::vector<uint8_t> encode;
  if (!present) {
    encode.resize(static_cast<size_t>(batch) * n);
    for (size_t j = 0; j < encode.size(); ++j) encode[j] = static_cast<int>(j % n) < k;
    present = encode.data();
  }
  // all sizes equal: exactly the mixed plan of that size (the uniform plan when the masks
  // are equal too)
  if (ragged_sizes_equal(batch, sizes))
    return rs_plan_create_mixed(ctx, device, k, m, sizes[0], batch, present, shards, out);
  Device* dev = ctx->device(device);
  if (!dev) return RS_E_ARG;
  RaggedTables rt;
  switch (build_ragged_tables(k, m, batch, sizes, present, rt)) {
    case RaggedError::kOk: break;
    case RaggedError::kNoData: return RS_E_NO_DATA;
    case RaggedError::kTooManyTiles: return RS_E_ARG;  // a grid past 2^31 - 1 tiles
    case RaggedError::kTooFewShards: return RS_E_TOO_FEW_SHARDS;
    case RaggedError::kSingular: return RS_E_SINGULAR;
  }
  auto plan = new_plan(device, *std::max_element(sizes, sizes + batch), batch);
  plan->mixed = std::make_unique<MixedPlan>();
  plan->fixed_form = kOrderRagged + RS_ORDER_CONSECUTIVE;
  MixedPlan& mp = *plan->mixed;
  mp.t = std::move(rt.mixed);
  mp.ragged = true;
  mp.any_tail = rt.any_tail;
  mp.ntiles = rt.ntiles;
  // every shard of every stripe is read, compared or written
  plan->bytes = rt.total * static_cast<uint64_t>(n);
  rc = upload_mixed(*plan, shards, &rt);
  if (rc) return rc;
  *out = plan.release();
  return RS_OK;
}

int rs_plan_create_required(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                            const uint8_t* present, const uint8_t* required,
                            uint8_t* const* shards, rs_plan** out) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || !sizes || !shards || !out || batch < 1) return RS_E_ARG;
  *out = nullptr;
  const int n = k + m;
  // nothing to leave out (no masks: every stripe an encode): exactly the ragged plan
  if (!required || !present || required_all_wanted(n, batch, present, required))
    return rs_plan_create_ragged(ctx, device, k, m, batch, sizes, present, shards, out);
  for (int b = 0; b < batch; ++b)
    if (sizes[b] == 0) return RS_E_NO_DATA;
  for (int b = 0; b < batch; ++b) {
    int np = 0;
    for (int i = 0; i < n; ++i) np += present[static_cast<size_t>(b) * n + i] != 0;
    if (np < k) return RS_E_TOO_FEW_SHARDS;
  }
  // one size, one (mask, wanted) pair: the uniform plan over the wanted rows
  if (ragged_sizes_equal(batch, sizes) && required_pairs_equal(n, batch, present, required))
    return create_uniform(ctx, device, k, m, sizes[0], batch, present, required, shards, out);
  Device* dev = ctx->device(device);
  if (!dev) return RS_E_ARG;
  RequiredTables rq;
  switch (build_required_tables(k, m, batch, sizes, present, required, rq)) {
    case RaggedError::kOk: break;
    case RaggedError::kNoData: return RS_E_NO_DATA;
    case RaggedError::kTooManyTiles: return RS_E_ARG;
    case RaggedError::kTooFewShards: return RS_E_TOO_FEW_SHARDS;
    case RaggedError::kSingular: return RS_E_SINGULAR;
  }
  auto plan = new_plan(device, *std::max_element(sizes, sizes + batch), batch);
  plan->mixed = std::make_unique<MixedPlan>();
  plan->fixed_form = kOrderRequired + RS_ORDER_CONSECUTIVE;
  MixedPlan& mp = *plan->mixed;
  mp.t = std::move(rq.mixed);
  mp.ragged = true;
  mp.some = true;
  // per stripe with a row: the k shards read, the rows written and the rows compared
  plan->bytes = rq.bytes;
  rc = upload_mixed(*plan, shards, nullptr, &rq);
  if (rc) return rc;
  *out = plan.release();
  return RS_OK;
}

void rs_plan_destroy(rs_plan* plan) {
  DeviceGuard dg;
  delete plan;
}

// ---- launches ---------------------------------------------------------------------------------

int rs_plan_launch(rs_plan* plan, void* stream) {
  return rs_plan_launch_timed(plan, stream, nullptr, nullptr);
}

int rs_plan_launch_timed(rs_plan* plan, void* stream, void* start_event, void* stop_event) {
  DeviceGuard dg;
  if (!plan) return RS_E_ARG;
  HIPCHK(hipSetDevice(plan->device));
  if (plan->S == 0 || plan_groups(*plan) == 0)  // nothing dispatches: the events still bracket this (empty) launch
    return record_empty(stream, start_event, stop_event);
  LaunchEvents ev;
  ev.start = static_cast<hipEvent_t>(start_event);
  ev.stop = static_cast<hipEvent_t>(stop_event);
  HIPCHK(plan_launch(*plan, static_cast<hipStream_t>(stream), plan->orders_snapshot(), ev));
  return RS_OK;
}

int rs_plan_launch_ceiling(rs_plan* plan, void* stream, int mode) {
  return rs_plan_launch_ceiling_timed(plan, stream, mode, nullptr, nullptr);
}

int rs_plan_launch_ceiling_timed(rs_plan* plan, void* stream, int mode, void* start_event,
                                 void* stop_event) {
  DeviceGuard dg;
  if (!plan || mode < 0 || mode > 8) return RS_E_ARG;
  if (!plan->has_orders()) return RS_E_ARG;  // no traffic ceilings for mixed and ragged plans
  // the product implements RS_CEIL_READ / RS_CEIL_WRITE; the other modes are the A/B build's
  // (tools/callfs_rs_ab.h)
  if (!kAbInstances && mode != RS_CEIL_READ && mode != RS_CEIL_WRITE) return RS_E_ARG;
  HIPCHK(hipSetDevice(plan->device));
  const std::vector<int> orders = plan->orders_snapshot();
  if (plan->S < 16)  // the ceilings cover whole 16-B vectors only: nothing dispatches
    return record_empty(stream, start_event, stop_event);
  LaunchEvents ev;
  ev.start = static_cast<hipEvent_t>(start_event);
  ev.stop = static_cast<hipEvent_t>(stop_event);
  const size_t ng = plan_groups(*plan);
  for (size_t gi = 0; gi < ng; ++gi) {
    const int order = gi < orders.size() ? orders[gi] : -1;
    HIPCHK(launch_ceiling(plan_group_args(*plan, gi), static_cast<hipStream_t>(stream), order, mode,
                          group_events(ev, gi, ng)));
  }
  return RS_OK;
}

// ---- tile orders --------------------------------------------------------------------------------

// Times every tile order each launch group's kernel offers and keeps the fastest. Which
// order HBM serves best varies between MI355X boxes by 1-2 points on the same shape
// (DESIGN.md §6.2 "Tile order"), so a plan that is launched many times measures it on the
// box it runs on, like a library autotuner, instead of trusting the rule alone. Each
// candidate gets `reps` back-to-back launches between two events, in three rounds with the
// candidate order rotated; the per-launch mean of the best round counts, and the rule's
// order is kept unless another is faster by more than 1 % (with 0.3 % the tuner sometimes
// left the rule for an order that then timed 0.5-1 % slower, round 3).
int rs_plan_tune(rs_plan* plan, void* stream, int reps, int* orders, int max_groups) {
  DeviceGuard dg;
  if (!plan || reps < 1 || max_groups < 0 || (max_groups > 0 && !orders)) return RS_E_ARG;
  if (!plan->has_orders()) {  // one form, one tile order: nothing to time
    for (int i = 0; i < max_groups; ++i) orders[i] = -1;
    return RS_OK;
  }
  HIPCHK(hipSetDevice(plan->device));
  auto s = static_cast<hipStream_t>(stream);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  HIPCHK(hipStreamIsCapturing(s, &cap));
  if (cap != hipStreamCaptureStatusNone) return RS_E_ARG;  // synchronous: not in a capture
  const Tables& t = *plan->tables;
  std::vector<int> chosen(t.groups.size(), -1);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPCHK(hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) {
    (void)hipEventDestroy(e0);
    return RS_E_HIP;
  }
  int rc = RS_OK;
  for (size_t gi = 0; gi < t.groups.size() && rc == RS_OK; ++gi) {
    const ApplyArgs a = plan_group_args(*plan, gi);
    std::vector<int> cand = order_candidates(a);
    // the bit-sliced orders only when the group's kernel compiles and loads here: a hiprtc
    // that fails on some box leaves the tuner (and the bench) on the nibble-table forms
    const Group& grp = t.groups[gi];
    const auto bs_order = [](int o) { return decode_order(o).family == Family::kBitslice; };
    if (std::any_of(cand.begin(), cand.end(), bs_order) &&
        (!grp.bsk || !grp.bsk->function(plan->device, /*wait=*/true)))
      cand.erase(std::remove_if(cand.begin(), cand.end(), bs_order), cand.end());
    if (cand.size() < 2) continue;
    std::vector<float> best(cand.size(), 1e30f);
    // warm-up in the rule's order first, by time: a chip that has just come out of other
    // (or no) work runs the bench shape up to 4 % slow for ~100 ms (bench.py at 5 vs 100
    // warm-up steps, profiles/r02/warmup/), and candidates timed during that ramp favour
    // whichever is timed last. Batches of `reps` launches until kTuneWarmMs of device
    // time have passed (at most kTuneWarmBatches batches).
    {
      float warm = 0;
      for (int b = 0; b < kTuneWarmBatches && warm < kTuneWarmMs && rc == RS_OK; ++b) {
        bool ok = hipEventRecord(e0, s) == hipSuccess;
        for (int r = 0; r < reps && ok; ++r) ok = launch_apply(a, s, false, cand[0]) == hipSuccess;
        float ms = 0;
        ok = ok && hipEventRecord(e1, s) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
             hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
        if (!ok) rc = RS_E_HIP;
        warm += ms;
      }
    }
    for (int round = 0; round < kTuneRounds && rc == RS_OK; ++round) {
      for (size_t j = 0; j < cand.size() && rc == RS_OK; ++j) {
        const size_t c = (j + round) % cand.size();
        // one untimed launch, then `reps` timed ones
        bool ok = launch_apply(a, s, false, cand[c]) == hipSuccess && hipEventRecord(e0, s) == hipSuccess;
        for (int r = 0; r < reps && ok; ++r) ok = launch_apply(a, s, false, cand[c]) == hipSuccess;
        ok = ok && hipEventRecord(e1, s) == hipSuccess && hipEventSynchronize(e1) == hipSuccess;
        float ms = 0;
        ok = ok && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
        if (!ok) {
          rc = RS_E_HIP;
          break;
        }
        best[c] = std::min(best[c], ms / static_cast<float>(reps));
      }
    }
    if (rc != RS_OK) break;
    size_t win = 0;  // cand[0] is the rule's order
    for (size_t c = 1; c < cand.size(); ++c)
      if (best[c] < best[win] * (win == 0 ? 1.0f - tune_bar() / 100.0f : 1.0f)) win = c;
    chosen[gi] = cand[win];
    record_tuned(a, chosen[gi]);  // later untuned launches of this shape take it
    if (tune_log()) {
      std::fprintf(stderr, "rs_plan_tune: group %zu (K=%d R=%d S=%zu batch=%d):", gi, a.K, a.R,
                   static_cast<size_t>(a.S), a.batch);
      for (size_t c = 0; c < cand.size(); ++c)
        std::fprintf(stderr, " order %d %.1f us%s", cand[c], best[c] * 1e3f, c == win ? " *" : "");
      std::fprintf(stderr, "\n");
    }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc != RS_OK) return rc;
  {
    std::lock_guard<std::mutex> g(plan->mu);
    plan->orders = chosen;
  }
  for (int i = 0; i < max_groups; ++i)
    orders[i] = static_cast<size_t>(i) < chosen.size() ? chosen[i] : -1;
  return RS_OK;
}

// Pins launch group i to orders[i] (-1: the rule), as rs_plan_tune would: the order must
// be one order_candidates offers for that group's kernel (RS_E_ARG otherwise, and nothing
// changes); a plan without tile orders accepts only -1. For orders tuned once and kept (a
// deployment's own shard layout), and for tests that run every instance.
int rs_plan_set_orders(rs_plan* plan, const int* orders, int n) {
  if (!plan || n < 0 || (n > 0 && !orders)) return RS_E_ARG;
  const size_t ng = plan_groups(*plan);
  if (static_cast<size_t>(n) > ng) return RS_E_ARG;
  std::vector<int> next(ng, -1);
  for (int gi = 0; gi < n; ++gi) {
    if (orders[gi] == -1) continue;
    if (!plan->has_orders()) return RS_E_ARG;
    const std::vector<int> cand = order_candidates(plan_group_args(*plan, gi), /*every_instance=*/true);
    if (std::find(cand.begin(), cand.end(), orders[gi]) == cand.end()) return RS_E_ARG;
    next[gi] = orders[gi];
  }
  std::lock_guard<std::mutex> g(plan->mu);
  plan->orders = next;
  return RS_OK;
}

int rs_tune_table_reset(const char* path) {
  tune_table().reset(path);
  return RS_OK;
}

int rs_tune_table_entries(void) { return static_cast<int>(tune_table().size()); }

int rs_plan_forms(const rs_plan* plan, int* forms, int max_groups) {
  if (!plan || max_groups < 0 || (max_groups > 0 && !forms)) return RS_E_ARG;
  const int ng = static_cast<int>(plan_groups(*plan));
  const std::vector<int> orders = plan->orders_snapshot();
  for (int gi = 0; gi < ng && gi < max_groups; ++gi) {
    const int order = static_cast<size_t>(gi) < orders.size() ? orders[gi] : -1;
    forms[gi] = plan->has_orders() ? launch_form(plan_group_args(*plan, gi), order) : plan->fixed_form;
  }
  return ng;
}

// ---- status and size ----------------------------------------------------------------------------

int rs_plan_stripe_status(rs_plan* plan, void* stream, int* flags) {
  DeviceGuard dg;
  if (!plan || !flags) return RS_E_ARG;
  HIPCHK(hipSetDevice(plan->device));
  auto s = static_cast<hipStream_t>(stream);
  auto* st = static_cast<uint8_t*>(plan->dmeta.p) + plan->status_off;
  const size_t bytes = sizeof(int) * static_cast<size_t>(plan->batch);
  HIPCHK(hipMemcpyAsync(flags, st, bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemsetAsync(st, 0, bytes, s));
  HIPCHK(hipStreamSynchronize(s));
  return RS_OK;
}

int rs_plan_status(rs_plan* plan, void* stream, int* corrupt) {
  if (!plan || !corrupt) return RS_E_ARG;
  std::vector<int> flags(static_cast<size_t>(plan->batch));
  const int rc = rs_plan_stripe_status(plan, stream, flags.data());
  if (rc) return rc;
  *corrupt = std::any_of(flags.begin(), flags.end(), [](int f) { return f != 0; });
  return RS_OK;
}

uint64_t rs_plan_bytes(const rs_plan* plan) { return plan ? plan->bytes : 0; }

int rs_plan_groups(const rs_plan* plan) { return plan ? static_cast<int>(plan_groups(*plan)) : 0; }

// ---- one-shot device calls ------------------------------------------------------------------------

int rs_encode_dev(rs_ctx* ctx, int device, int k, int m, size_t S, int batch,
                  uint8_t* const* shards, void* stream) {
  return one_shot(ctx, device, k, m, S, batch, nullptr, shards, stream);
}

int rs_decode_dev(rs_ctx* ctx, int device, int k, int m, size_t S, int batch,
                  const uint8_t* present, uint8_t* const* shards, void* stream) {
  if (!present) return RS_E_ARG;
  return one_shot(ctx, device, k, m, S, batch, present, shards, stream);
}

int rs_decode_dev_mixed(rs_ctx* ctx, int device, int k, int m, size_t S, int batch,
                        const uint8_t* present, uint8_t* const* shards, void* stream) {
  if (!present) return RS_E_ARG;
  rs_plan* p = nullptr;
  const int rc = rs_plan_create_mixed(ctx, device, k, m, S, batch, present, shards, &p);
  if (rc) return rc;
  return launch_once(p, stream);
}

int rs_decode_dev_ragged(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                         const uint8_t* present, uint8_t* const* shards, void* stream) {
  rs_plan* p = nullptr;
  const int rc = rs_plan_create_ragged(ctx, device, k, m, batch, sizes, present, shards, &p);
  if (rc) return rc;
  return launch_once(p, stream);
}

int rs_decode_dev_required(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                           const uint8_t* present, const uint8_t* required,
                           uint8_t* const* shards, void* stream) {
  rs_plan* p = nullptr;
  const int rc = rs_plan_create_required(ctx, device, k, m, batch, sizes, present, required,
                                         shards, &p);
  if (rc) return rc;
  return launch_once(p, stream);
}

}  // extern "C"
