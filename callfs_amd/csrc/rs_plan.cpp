// Device-resident plans of the C ABI (include/callfs_rs.h): tables uploaded once for
// repeated, graph-capturable launches over shards in device memory -- uniform plans (one
// erasure pattern, one shard size: every kernel form and tile order), mixed plans (a
// pattern per stripe), ragged plans (a shard size per stripe too, §5.9) and
// required plans (only the missing shards a caller wants, §5.10) and locate plans (which shard
// is corrupt, §5.12), which share one layout, one upload and one constructor tail -- the
// tile-order tuner and the one-shot device calls built on them.
#include <cstdio>

#include "decode_check_tables.hpp"
#include "decode_idx_tables.hpp"
#include "decode_repair_tables.hpp"
#include "feed_tables.hpp"
#include "locate_tables.hpp"
#include "mixed_tables.hpp"
#include "ragged_tables.hpp"
#include "rs_internal.hpp"
#include "tune_table.hpp"
#include "update_tables.hpp"

using namespace callfs;

static_assert(kRaggedTileVecs == kRaggedLaunchTileVecs, "the tile map counts the kernel's tiles");

// A plan with per-stripe tables (`tables` of rs_plan is null): the pattern tables and where each
// piece sits in the plan's device buffer. A mixed plan (rs_plan_create_mixed) has one shard size
// and no tile map. A ragged plan (rs_plan_create_ragged) adds the stripes' sizes and one tile map
// (ragged_tables.hpp) that every launch group names; the plan's S is the largest shard size
// (never 0). A required plan (rs_plan_create_required) is a ragged plan whose patterns have their
// own row counts: every launch group has its own tile map and launches with the patterns' row
// counts inside it. A locate plan (rs_plan_create_locate; rs_plan_create_correct's correct plan
// is one too, with `correct` set) is a required plan with nothing
// wanted, cut to its first launch group, plus what the classification reads (the shared log / exp
// block and a block per pattern) and the per-stripe, per-shard counts it adds into.
enum class PlanKind { kMixed, kRagged, kRequired, kLocate };

struct MixedPlan {
  MixedTables t;
  PlanKind kind = PlanKind::kMixed;
  size_t in_off = 0, pat_off = 0, size_off = 0;
  struct Group {
    size_t out_off, vmask_off, arena_off, nrows_off;
    // the tile map the group launches with (none for a mixed plan)
    size_t tile0_off = 0, tile_stripe_off = 0;
    uint32_t ntiles = 0;
    bool any_tail = false;  // some stripe of the map has a size that is no multiple of 16
  };
  std::vector<Group> groups;  // per launch group of `t`
  // a locate plan's pieces: locate_tables.hpp's blocks and the batch * (k + m + 1) counts
  size_t gf_off = 0, loc_off = 0, loc_stride = 0, counts_off = 0;
  int max_errors = 1;  // 2: a pair plan (rs_plan_create_locate_ex)
  // a correct plan (rs_plan_create_correct): a locate plan in every piece, whose
  // launches repair what they blame
  bool correct = false;
};

// An update plan (rs_plan_create_update): where the pieces of
// update_tables.hpp sit in the plan's device buffer. One tile map, over the stripes with a
// changed shard, for every launch group; no launch group at all when nothing changed.
// A decode-idx plan (rs_plan_create_decode_idx, §5.14) is laid out the same way from
// decode_idx_tables.hpp: single sources, and per launch group the patterns' row counts. A
// decode-check plan (rs_plan_create_decode_check, §5.15) is a decode-idx plan from
// decode_check_tables.hpp that also holds per launch group the patterns' check rows; a final one
// launches the kernel that tests them. A decode-repair plan (rs_plan_create_decode_repair, §5.16)
// is a final decode-check plan from decode_repair_tables.hpp plus the locate blocks, the fix
// pointer table and the batch * (k + m + 1) counts; it launches the kernel that repairs.
struct UpdatePlan {
  bool pair = true;  // sources are (old, new) pairs; false: EncodeIdx mode
  bool decode_idx = false, store = false;  // a decode-idx plan, and whether it stores or merges
  bool check_final = false;                // a final decode-check plan (decode_idx is set too)
  int cmax = 0;
  size_t in_off = 0, pat_off = 0, nsrc_off = 0, size_off = 0, tile0_off = 0, tile_stripe_off = 0;
  uint32_t ntiles = 0;
  bool any_tail = false;
  struct Group {
    int R;
    size_t out_off, arena_off;
    uint32_t tab_stride;
    size_t nrows_off = 0;  // a decode-idx plan's [P] row counts
    size_t cmask_off = 0;  // a decode-check plan's [P] check-row masks (read by a final one)
  };
  std::vector<Group> groups;
  // a decode-repair plan's pieces (check_final is set too)
  bool repair = false;
  int k = 0, m = 0;
  size_t gf_off = 0, loc_off = 0, loc_stride = 0, fix_off = 0, counts_off = 0;
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
  // An update plan (`tables` and `mixed` are null): `fixed_form` too, and no status to flag.
  std::unique_ptr<UpdatePlan> update;
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

// A feed object (rs_feed_create): feed_tables.hpp's arena in one device buffer
// behind the table of row pointers, uploaded once. A launch picks the delivered shard's block.
struct rs_feed {
  int device = 0;
  size_t S = 0;
  FeedTables t;
  std::vector<uint8_t*> rows;  // compared, then wanted
  DevBuf dmeta;                // [kFeedMaxRows] row pointers, then the arena
  ~rs_feed() {
    if (dmeta.p) (void)hipSetDevice(device);  // the buffer is freed on the object's device
  }
};

// An absorb object (rs_absorb_create): absorb_tables.hpp's arena in one device
// buffer behind the table of row pointers, uploaded once. A launch plans its range on the host
// and passes the plan by value.
struct rs_absorb {
  int device = 0;
  size_t S = 0;
  AbsorbTables t;
  std::vector<uint8_t*> rows;  // parity row j
  DevBuf dmeta;                // [kAbsorbMaxRows] row pointers, then the arena
  std::mutex mu;               // guards scratch
  std::vector<OverwriteInterval> scratch;
  ~rs_absorb() {
    if (dmeta.p) (void)hipSetDevice(device);  // the buffer is freed on the object's device
  }
};

namespace {

// ---- what differs between uniform, mixed and ragged plans -------------------------------

size_t plan_groups(const rs_plan& plan) {
  if (plan.update) return plan.update->groups.size();
  return plan.mixed ? plan.mixed->t.groups.size() : plan.tables->groups.size();
}

// The arguments of launch group gi. A plan with per-stripe tables gives them as *x (the
// MixedArgs fields, and the group's tile map unless the plan is a mixed one) and, for a required
// plan, the patterns' row counts as *nrows (null otherwise).
ApplyArgs plan_group_args(const rs_plan& plan, size_t gi, RaggedArgs* x = nullptr,
                          const uint32_t** nrows = nullptr) {
  auto* d = static_cast<uint8_t*>(plan.dmeta.p);
  if (!plan.mixed)
    return group_args(*plan.tables, plan.layout, gi, plan.batch, d, plan.S, 1, plan.hint);
  const MixedPlan& mp = *plan.mixed;
  const MixedGroup& g = mp.t.groups[gi];
  const MixedPlan::Group& at = mp.groups[gi];
  ApplyArgs a{};
  a.in_tab = reinterpret_cast<const uint8_t* const*>(d + mp.in_off);
  a.out_tab = reinterpret_cast<uint8_t* const*>(d + at.out_off);
  a.ltabs = d + at.arena_off;
  a.S = plan.S;
  a.status = reinterpret_cast<int*>(d + plan.status_off);
  a.status_stride = 1;
  a.K = mp.t.k;
  a.R = g.R;
  a.batch = plan.batch;
  if (x) {
    x->pat = reinterpret_cast<const uint32_t*>(d + mp.pat_off);
    x->vmask = reinterpret_cast<const uint32_t*>(d + at.vmask_off);
    x->tab_stride = static_cast<uint32_t>(g.tab_stride);
    if (mp.kind != PlanKind::kMixed) {
      x->size = reinterpret_cast<const uint64_t*>(d + mp.size_off);
      x->tile0 = reinterpret_cast<const uint32_t*>(d + at.tile0_off);
      x->tile_stripe = reinterpret_cast<const uint32_t*>(d + at.tile_stripe_off);
      x->ntiles = at.ntiles;
    }
  }
  if (nrows)
    *nrows = mp.kind == PlanKind::kRequired || mp.kind == PlanKind::kLocate
                 ? reinterpret_cast<const uint32_t*>(d + at.nrows_off)
                 : nullptr;
  return a;
}

// Every launch group on stream s; ev as for launch_groups. `orders` counts for plans that
// have tile orders.
hipError_t plan_launch(const rs_plan& plan, hipStream_t s, const std::vector<int>& orders,
                       LaunchEvents ev) {
  if (plan.update) {
    const UpdatePlan& up = *plan.update;
    auto* d = static_cast<uint8_t*>(plan.dmeta.p);
    const size_t ng = up.groups.size();
    for (size_t gi = 0; gi < ng; ++gi) {
      const UpdatePlan::Group& g = up.groups[gi];
      ApplyArgs a{};
      a.in_tab = reinterpret_cast<const uint8_t* const*>(d + up.in_off);
      a.out_tab = reinterpret_cast<uint8_t* const*>(d + g.out_off);
      a.ltabs = d + g.arena_off;
      a.K = up.cmax;
      a.R = g.R;
      a.batch = plan.batch;
      UpdateArgs x{};
      x.pat = reinterpret_cast<const uint32_t*>(d + up.pat_off);
      x.nsrc = reinterpret_cast<const uint32_t*>(d + up.nsrc_off);
      x.size = reinterpret_cast<const uint64_t*>(d + up.size_off);
      x.tile0 = reinterpret_cast<const uint32_t*>(d + up.tile0_off);
      x.tile_stripe = reinterpret_cast<const uint32_t*>(d + up.tile_stripe_off);
      x.tab_stride = g.tab_stride;
      x.ntiles = up.ntiles;
      x.in_stride = static_cast<uint32_t>(up.cmax) * (up.pair ? 2u : 1u);
      const MergeArgs xm{x, reinterpret_cast<const uint32_t*>(d + g.nrows_off)};
      hipError_t e;
      if (up.repair) {
        a.status = reinterpret_cast<int*>(d + plan.status_off);
        a.status_stride = 1;
        const RepairArgs xr{CheckArgs{xm, reinterpret_cast<const uint32_t*>(d + g.cmask_off)},
                            d + up.gf_off,
                            d + up.loc_off,
                            reinterpret_cast<uint64_t*>(d + up.counts_off),
                            reinterpret_cast<uint8_t* const*>(d + up.fix_off),
                            static_cast<uint32_t>(up.loc_stride),
                            static_cast<uint32_t>(up.k + up.m + 1),
                            up.k};
        e = launch_decode_repair(a, xr, up.store, up.any_tail, s, group_events(ev, gi, ng));
      } else if (up.check_final) {
        a.status = reinterpret_cast<int*>(d + plan.status_off);
        a.status_stride = 1;
        e = launch_decode_check(a, CheckArgs{xm, reinterpret_cast<const uint32_t*>(d + g.cmask_off)}, up.store,
                                up.any_tail, s, group_events(ev, gi, ng));
      } else if (up.decode_idx) {
        e = launch_decode_idx(a, xm, up.store, up.any_tail, s, group_events(ev, gi, ng));
      } else {
        e = launch_update(a, x, up.pair, up.any_tail, s, group_events(ev, gi, ng));
      }
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  if (!plan.mixed)
    return launch_groups(*plan.tables, plan.layout, plan.batch, static_cast<uint8_t*>(plan.dmeta.p),
                         plan.S, s, /*status_stride=*/1, plan.hint, &orders, ev);
  const size_t ng = plan_groups(plan);
  for (size_t gi = 0; gi < ng; ++gi) {
    RaggedArgs r{};
    const uint32_t* nrows = nullptr;
    const ApplyArgs a = plan_group_args(plan, gi, &r, &nrows);
    const LaunchEvents g = group_events(ev, gi, ng);
    const MixedPlan& mp = *plan.mixed;
    hipError_t e;
    if (mp.kind == PlanKind::kMixed) {
      e = launch_mixed(a, MixedArgs{r.pat, r.vmask, r.tab_stride}, s, g);
    } else if (mp.kind == PlanKind::kLocate) {
      auto* d = static_cast<uint8_t*>(plan.dmeta.p);
      const LocateArgs x{r, nrows, d + mp.gf_off, d + mp.loc_off,
                         reinterpret_cast<uint64_t*>(d + mp.counts_off),
                         static_cast<uint32_t>(mp.loc_stride), static_cast<uint32_t>(mp.t.k + mp.t.m + 1)};
      e = mp.correct ? launch_correct(a, x, mp.groups[gi].any_tail, s, g)
                     : launch_locate(a, x, mp.groups[gi].any_tail, s, g, mp.max_errors);
    } else {
      e = launch_ragged(a, r, nrows, mp.groups[gi].any_tail, s, g);
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ---- plan construction --------------------------------------------------------------------

// The head of every constructor: the profile, then the arguments (`given`: the pointers that
// constructor requires).
int check_plan_args(rs_ctx* ctx, int k, int m, int batch, bool given, rs_plan** out) {
  if (const int rc = check_profile(k, m)) return rc;
  if (!ctx || !given || !out || batch < 1) return RS_E_ARG;
  *out = nullptr;
  return RS_OK;
}

// What every stripe needs, whichever path the plan takes: a shard size (sizes nullable; upstream
// Encode: ErrShardNoData), then k present shards (present nullable).
int check_stripes(int k, int n, int batch, const size_t* sizes, const uint8_t* present) {
  for (int b = 0; sizes && b < batch; ++b)
    if (sizes[b] == 0) return RS_E_NO_DATA;
  for (int b = 0; present && b < batch; ++b) {
    int np = 0;
    for (int i = 0; i < n; ++i) np += present[static_cast<size_t>(b) * n + i] != 0;
    if (np < k) return RS_E_TOO_FEW_SHARDS;
  }
  return RS_OK;
}

int table_status(TableError e) {
  switch (e) {
    case TableError::kOk: break;
    case TableError::kNoData: return RS_E_NO_DATA;
    case TableError::kTooManyTiles: return RS_E_ARG;  // a grid past 2^31 - 1 tiles
    case TableError::kTooFewShards: return RS_E_TOO_FEW_SHARDS;
    case TableError::kSingular: return RS_E_SINGULAR;
  }
  return RS_OK;
}

int decode_idx_status(DecodeIdxError e) {
  switch (e) {
    case DecodeIdxError::kOk: break;
    case DecodeIdxError::kArg: return RS_E_ARG;
    case DecodeIdxError::kTooFewShards: return RS_E_TOO_FEW_SHARDS;
    case DecodeIdxError::kNoData: return RS_E_NO_DATA;
    case DecodeIdxError::kTooManyTiles: return RS_E_ARG;  // a grid past 2^31 - 1 tiles
    case DecodeIdxError::kSingular: return RS_E_SINGULAR;
  }
  return RS_OK;
}

std::unique_ptr<rs_plan> new_plan(int device, size_t S, int batch) {
  auto plan = std::make_unique<rs_plan>();
  plan->device = device;
  plan->S = S;
  plan->batch = batch;
  return plan;
}

// rs_plan_create's body. wanted (k+m flags, or null: every missing shard): the missing shards
// that get a row; a plan with no row at all has no launch group.
int create_uniform(rs_ctx* ctx, int device, int k, int m, size_t S, int batch,
                   const uint8_t* present, const uint8_t* wanted, uint8_t* const* shards,
                   rs_plan** out) {
  DeviceGuard dg;
  int rc = check_plan_args(ctx, k, m, batch, shards, out);
  if (rc) return rc;
  if (!ctx->device(device)) return RS_E_ARG;
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

// Lays out and uploads the device buffer of a plan with per-stripe tables (plan.mixed->t built,
// plan.device and plan.batch set): the status words, the shard-pointer tables, pat and per launch
// group the compare masks, the table arena and the patterns' row counts, each piece 256-B
// aligned. With `rt` (a ragged or required plan) also the stripes' sizes and the tile maps, and
// every launch group is given its own. An out_tab slot at or past a stripe's row count holds
// null, and a shard no row names is in no table. With `lt` (a locate plan; rt is its ragged
// part) also the classification's blocks and the zeroed counts.
int upload_mixed(rs_plan& plan, uint8_t* const* shards, const RaggedTables* rt,
                 const LocateTables* lt = nullptr) {
  MixedPlan& mp = *plan.mixed;
  const int k = mp.t.k, n = mp.t.k + mp.t.m, batch = plan.batch;
  Packer pk;
  const size_t P = mp.t.patterns.size();
  plan.status_off = pk.take(sizeof(int) * static_cast<size_t>(batch));
  mp.in_off = pk.take(sizeof(void*) * static_cast<size_t>(batch) * k);
  mp.pat_off = pk.take(sizeof(uint32_t) * static_cast<size_t>(batch));
  for (const MixedGroup& g : mp.t.groups) {
    MixedPlan::Group at{};
    at.out_off = pk.take(sizeof(void*) * static_cast<size_t>(batch) * g.R);
    at.vmask_off = pk.take(sizeof(uint32_t) * P);
    at.arena_off = pk.take(g.arena.size());
    at.nrows_off = pk.take(sizeof(uint32_t) * P);
    mp.groups.push_back(at);
  }
  std::vector<size_t> tile0_off, tile_stripe_off;  // per map of rt
  if (rt) {
    mp.size_off = pk.take(sizeof(uint64_t) * rt->size.size());
    for (const TileMap& tm : rt->maps) {
      tile0_off.push_back(pk.take(sizeof(uint32_t) * tm.tile0.size()));
      tile_stripe_off.push_back(pk.take(sizeof(uint32_t) * std::max<size_t>(1, tm.tile_stripe.size())));
    }
  }
  if (lt) {
    mp.gf_off = pk.take(lt->gf.size());
    mp.loc_stride = lt->stride;
    mp.max_errors = lt->max_errors;
    mp.loc_off = pk.take(std::max<size_t>(1, lt->loc.size()));
    mp.counts_off = pk.take(sizeof(uint64_t) * static_cast<size_t>(batch) * (n + 1));
  }
  std::vector<uint8_t> h(pk.off, 0);
  auto put = [&](size_t off, const auto& v) {
    if (!v.empty()) std::memcpy(h.data() + off, v.data(), sizeof(v[0]) * v.size());
  };
  if (lt) {
    put(mp.gf_off, lt->gf);
    put(mp.loc_off, lt->loc);
  }
  auto shard_ptr = [&](int b, int i) { return shards[static_cast<size_t>(b) * n + i]; };
  auto* in = reinterpret_cast<const uint8_t**>(h.data() + mp.in_off);
  for (int b = 0; b < batch; ++b) {
    const MixedPattern& pt = mp.t.patterns[mp.t.pat[b]];
    for (int i = 0; i < k; ++i) in[static_cast<size_t>(b) * k + i] = shard_ptr(b, pt.valid[i]);
  }
  put(mp.pat_off, mp.t.pat);
  for (size_t gi = 0; gi < mp.t.groups.size(); ++gi) {
    const MixedGroup& g = mp.t.groups[gi];
    MixedPlan::Group& at = mp.groups[gi];
    auto* o = reinterpret_cast<uint8_t**>(h.data() + at.out_off);
    for (int b = 0; b < batch; ++b) {
      const MixedPattern& pt = mp.t.patterns[mp.t.pat[b]];
      for (int r = 0; r < g.R; ++r)
        o[static_cast<size_t>(b) * g.R + r] =
            static_cast<size_t>(g.row0 + r) < pt.rows.size() ? shard_ptr(b, pt.rows[g.row0 + r]) : nullptr;
    }
    put(at.vmask_off, g.vmask);
    put(at.arena_off, g.arena);
    put(at.nrows_off, g.nrows);
    if (rt) {
      const size_t mi = rt->maps.size() == 1 ? 0 : gi;
      at.tile0_off = tile0_off[mi];
      at.tile_stripe_off = tile_stripe_off[mi];
      at.ntiles = rt->maps[mi].ntiles;
      at.any_tail = rt->maps[mi].any_tail;
    }
  }
  if (rt) {
    put(mp.size_off, rt->size);
    for (size_t mi = 0; mi < rt->maps.size(); ++mi) {
      put(tile0_off[mi], rt->maps[mi].tile0);
      put(tile_stripe_off[mi], rt->maps[mi].tile_stripe);
    }
  }
  if (const int rc = upload(plan.dmeta, plan.device, h.data(), h.size())) return rc;
  // the device copy is all a launch reads: the host arenas can go
  for (MixedGroup& g : mp.t.groups) std::vector<uint8_t>().swap(g.arena);
  return RS_OK;
}

// The tail of the three constructors of plans with per-stripe tables, once their routes to
// simpler plans are not taken: the tables of `kind`, the plan and its device buffer. sizes and
// required count for ragged and required plans, S for a mixed one.
int create_tabled(rs_ctx* ctx, int device, int k, int m, PlanKind kind, size_t S, int batch,
                  const size_t* sizes, const uint8_t* present, const uint8_t* required,
                  uint8_t* const* shards, rs_plan** out, int max_errors = 1, bool correct = false) {
  if (!ctx->device(device)) return RS_E_ARG;
  const bool sized = kind != PlanKind::kMixed;
  LocateTables lt;
  RaggedTables& rt = lt.ragged;
  if (const int rc = table_status(kind == PlanKind::kLocate ? build_locate_tables(k, m, batch, sizes, present, lt, max_errors)
                                  : sized ? build_ragged_tables(k, m, batch, sizes, present, required, rt)
                                          : build_mixed_tables(k, m, batch, present, nullptr, rt.mixed)))
    return rc;
  auto plan = new_plan(device, sized ? *std::max_element(sizes, sizes + batch) : S, batch);
  plan->mixed = std::make_unique<MixedPlan>();
  plan->mixed->kind = kind;
  plan->mixed->correct = correct;
  plan->mixed->t = std::move(rt.mixed);
  plan->fixed_form = RS_ORDER_CONSECUTIVE + (kind == PlanKind::kMixed      ? kOrderMixed
                                             : kind == PlanKind::kRagged   ? kOrderRagged
                                             : kind == PlanKind::kRequired ? kOrderRequired
                                             : correct                     ? kOrderCorrect
                                                                           : kOrderLocate);
  // per stripe with a row: the k shards read, the rows written and the rows compared. Every
  // stripe of a mixed plan has m rows: n shards of S bytes each.
  plan->bytes = sized ? rt.bytes : static_cast<uint64_t>(batch) * S * static_cast<uint64_t>(k + m);
  if (const int rc = upload_mixed(*plan, shards, sized ? &rt : nullptr, kind == PlanKind::kLocate ? &lt : nullptr))
    return rc;
  *out = plan.release();
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

// The one-shot calls: create(&plan), launch, status, free; RS_E_CORRUPT when a stripe mismatched.
template <class Create>
int one_shot(Create create, void* stream) {
  rs_plan* p = nullptr;
  int rc = create(&p);
  if (rc) return rc;
  rc = rs_plan_launch(p, stream);
  int corrupt = 0;
  if (!rc) rc = rs_plan_status(p, stream, &corrupt);
  rs_plan_destroy(p);
  if (!rc && corrupt) rc = RS_E_CORRUPT;
  return rc;
}

const std::vector<int>& pattern_rows(const DecodeIdxPattern& p) { return p.wanted; }
const std::vector<int>& pattern_rows(const DecodeCheckPattern& p) { return p.rows; }
const std::vector<uint32_t>* group_cmask(const DecodeIdxGroup&) { return nullptr; }
const std::vector<uint32_t>* group_cmask(const DecodeCheckGroup& g) { return &g.cmask; }

// The body of the decode-idx and decode-check constructors once the tables stand: the plan's
// layout, its pointer tables and the upload. T: DecodeIdxTables or DecodeCheckTables; row(at):
// the pointer of the row at entry at = b * n + i (a wanted shard, or a check accumulator). With
// `rep` (a decode-repair plan; t is its decode-check part) also the shared log / exp block, the
// patterns' locate blocks, the fix pointers by position (`fix`: batch * n, null allowed) and the
// zeroed counts, each piece 256-B aligned.
template <class T, class Row>
int finish_decode_plan(int device, const T& t, const size_t* sizes, const uint8_t* const* input, Row row,
                       bool store, bool check_final, uint64_t bytes, rs_plan** out,
                       const DecodeRepairTables* rep = nullptr, uint8_t* const* fix = nullptr) {
  const int batch = t.batch, n = t.k + t.m;
  size_t smax = 0;
  for (int b = 0; b < batch; ++b)
    if (t.has[static_cast<size_t>(b)]) smax = std::max(smax, sizes[b]);
  auto plan = new_plan(device, smax, batch);
  plan->update = std::make_unique<UpdatePlan>();
  UpdatePlan& up = *plan->update;
  up.pair = false;
  up.decode_idx = true;
  up.store = store;
  up.check_final = check_final;
  up.cmax = t.cmax;
  up.ntiles = t.map.ntiles;
  up.any_tail = t.map.any_tail;
  plan->fixed_form = RS_ORDER_CONSECUTIVE + (rep           ? kOrderDecodeRepair
                                             : check_final ? kOrderDecodeCheck
                                                           : kOrderDecodeIdx);
  plan->bytes = bytes;
  const size_t stride = static_cast<size_t>(t.cmax);
  const size_t P = t.patterns.size();
  Packer pk;
  plan->status_off = pk.take(sizeof(int) * static_cast<size_t>(batch));
  up.in_off = pk.take(sizeof(void*) * std::max<size_t>(1, static_cast<size_t>(batch) * stride));
  up.pat_off = pk.take(sizeof(uint32_t) * static_cast<size_t>(batch));
  up.nsrc_off = pk.take(sizeof(uint32_t) * std::max<size_t>(1, P));
  up.size_off = pk.take(sizeof(uint64_t) * static_cast<size_t>(batch));
  up.tile0_off = pk.take(sizeof(uint32_t) * t.map.tile0.size());
  up.tile_stripe_off = pk.take(sizeof(uint32_t) * std::max<size_t>(1, t.map.tile_stripe.size()));
  for (const auto& g : t.groups) {
    UpdatePlan::Group at{g.R, pk.take(sizeof(void*) * static_cast<size_t>(batch) * g.R),
                         pk.take(std::max<size_t>(1, g.arena.size())), static_cast<uint32_t>(g.tab_stride)};
    at.nrows_off = pk.take(sizeof(uint32_t) * P);
    if (group_cmask(g)) at.cmask_off = pk.take(sizeof(uint32_t) * P);
    up.groups.push_back(at);
  }
  if (rep) {
    up.repair = true;
    up.k = t.k;
    up.m = t.m;
    up.gf_off = pk.take(rep->gf.size());
    up.loc_stride = rep->stride;
    up.loc_off = pk.take(std::max<size_t>(1, rep->loc.size()));
    up.fix_off = pk.take(sizeof(void*) * static_cast<size_t>(batch) * fix_slots(t.k));
    up.counts_off = pk.take(sizeof(uint64_t) * static_cast<size_t>(batch) * (n + 1));
  }
  std::vector<uint8_t> h(pk.off, 0);
  auto put = [&](size_t off, const auto& v) {
    if (!v.empty()) std::memcpy(h.data() + off, v.data(), sizeof(v[0]) * v.size());
  };
  if (rep) {
    put(up.gf_off, rep->gf);
    put(up.loc_off, rep->loc);
    // fix pointers of stripe b by position: its expected shards, then its compared shards
    auto* f = reinterpret_cast<uint8_t**>(h.data() + up.fix_off);
    for (int b = 0; b < batch; ++b) {
      if (!t.has[static_cast<size_t>(b)]) continue;
      const uint32_t p = t.pat[static_cast<size_t>(b)];
      const auto& pt = t.patterns[p];
      uint8_t** fb = f + static_cast<size_t>(b) * fix_slots(t.k);
      for (int j = 0; j < t.k; ++j) fb[j] = fix[static_cast<size_t>(b) * n + pt.expect[static_cast<size_t>(j)]];
      for (uint32_t x = 0; x < rep->nchk[p]; ++x)
        fb[t.k + x] = fix[static_cast<size_t>(b) * n + pattern_rows(pt)[x]];
    }
  }
  // sources of stripe b: its pattern's delivered shards in ascending order; slots past its
  // source count, and every slot of a stripe in no launch, stay null and unread
  auto* in = reinterpret_cast<const uint8_t**>(h.data() + up.in_off);
  for (int b = 0; b < batch; ++b) {
    if (!t.has[static_cast<size_t>(b)]) continue;
    const std::vector<int>& idx = t.patterns[t.pat[static_cast<size_t>(b)]].delivered;
    for (size_t c = 0; c < idx.size(); ++c) in[b * stride + c] = input[static_cast<size_t>(b) * n + idx[c]];
  }
  put(up.pat_off, t.pat);
  put(up.nsrc_off, t.nsrc);
  put(up.size_off, t.size);
  put(up.tile0_off, t.map.tile0);
  put(up.tile_stripe_off, t.map.tile_stripe);
  for (size_t gi = 0; gi < t.groups.size(); ++gi) {
    const auto& g = t.groups[gi];
    // rows of stripe b in this group: its pattern's rows row0 .. row0 + nrows[p]
    auto* o = reinterpret_cast<uint8_t**>(h.data() + up.groups[gi].out_off);
    for (int b = 0; b < batch; ++b) {
      if (!t.has[static_cast<size_t>(b)]) continue;
      const uint32_t p = t.pat[static_cast<size_t>(b)];
      const std::vector<int>& w = pattern_rows(t.patterns[p]);
      for (uint32_t r = 0; r < g.nrows[p]; ++r)
        o[static_cast<size_t>(b) * g.R + r] = row(static_cast<size_t>(b) * n + w[g.row0 + r]);
    }
    put(up.groups[gi].arena_off, g.arena);
    put(up.groups[gi].nrows_off, g.nrows);
    if (const std::vector<uint32_t>* cm = group_cmask(g)) put(up.groups[gi].cmask_off, *cm);
  }
  if (const int rc = upload(plan->dmeta, device, h.data(), h.size())) return rc;
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
  int rc = check_plan_args(ctx, k, m, batch, shards && present, out);
  if (!rc) rc = check_stripes(k, k + m, batch, nullptr, present);
  if (rc) return rc;
  // all masks equal: exactly the uniform plan (its forms, bit-sliced kernels included)
  if (required_pairs_equal(k + m, batch, present, nullptr))
    return rs_plan_create(ctx, device, k, m, S, batch, present, shards, out);
  return create_tabled(ctx, device, k, m, PlanKind::kMixed, S, batch, nullptr, present, nullptr, shards, out);
}

int rs_plan_create_ragged(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                          const uint8_t* present, uint8_t* const* shards, rs_plan** out) {
  DeviceGuard dg;
  int rc = check_plan_args(ctx, k, m, batch, sizes && shards, out);
  if (!rc) rc = check_stripes(k, k + m, batch, sizes, nullptr);
  if (rc) return rc;
  const int n = k + m;
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
  return create_tabled(ctx, device, k, m, PlanKind::kRagged, 0, batch, sizes, present, nullptr, shards, out);
}

int rs_plan_create_required(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                            const uint8_t* present, const uint8_t* required,
                            uint8_t* const* shards, rs_plan** out) {
  DeviceGuard dg;
  int rc = check_plan_args(ctx, k, m, batch, sizes && shards, out);
  if (rc) return rc;
  const int n = k + m;
  // nothing to leave out (no masks: every stripe an encode): exactly the ragged plan
  if (!present || required_all_wanted(n, batch, present, required))
    return rs_plan_create_ragged(ctx, device, k, m, batch, sizes, present, shards, out);
  if ((rc = check_stripes(k, n, batch, sizes, present))) return rc;
  // one size, one (mask, wanted) pair: the uniform plan over the wanted rows
  if (ragged_sizes_equal(batch, sizes) && required_pairs_equal(n, batch, present, required))
    return create_uniform(ctx, device, k, m, sizes[0], batch, present, required, shards, out);
  return create_tabled(ctx, device, k, m, PlanKind::kRequired, 0, batch, sizes, present, required, shards, out);
}

int rs_plan_create_locate(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                          const uint8_t* present, uint8_t* const* shards, rs_plan** out) {
  return rs_plan_create_locate_ex(ctx, device, k, m, batch, sizes, present, shards, 1, out);
}

int rs_plan_create_locate_ex(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                             const uint8_t* present, uint8_t* const* shards, int max_errors,
                             rs_plan** out) {
  DeviceGuard dg;
  int rc = check_plan_args(ctx, k, m, batch, sizes && shards && max_errors >= 1, out);
  if (!rc && max_errors > 2) rc = RS_E_UNSUPPORTED;
  if (!rc) rc = check_stripes(k, k + m, batch, sizes, nullptr);
  if (rc) return rc;
  // no masks: every shard of every stripe is present
  std::vector<uint8_t> all;
  if (!present) {
    all.assign(static_cast<size_t>(batch) * (k + m), 1);
    present = all.data();
  }
  // (no route to a simpler plan: only this kind counts)
  return create_tabled(ctx, device, k, m, PlanKind::kLocate, 0, batch, sizes, present, nullptr, shards, out,
                       max_errors);
}

// A locate plan (max_errors 1: the same checks in the same order, the same tables) that
// launches rs_apply_correct.
int rs_plan_create_correct(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                           const uint8_t* present, uint8_t* const* shards, rs_plan** out) {
  DeviceGuard dg;
  int rc = check_plan_args(ctx, k, m, batch, sizes && shards, out);
  if (!rc) rc = check_stripes(k, k + m, batch, sizes, nullptr);
  if (rc) return rc;
  std::vector<uint8_t> all;
  if (!present) {
    all.assign(static_cast<size_t>(batch) * (k + m), 1);
    present = all.data();
  }
  return create_tabled(ctx, device, k, m, PlanKind::kLocate, 0, batch, sizes, present, nullptr, shards, out, 1,
                       /*correct=*/true);
}

int rs_plan_create_update(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                          const uint8_t* changed, const uint8_t* const* old_data,
                          const uint8_t* const* new_data, uint8_t* const* parity, rs_plan** out) {
  DeviceGuard dg;
  // (old_data NULL is EncodeIdx mode, not an error)
  int rc = check_plan_args(ctx, k, m, batch, sizes && changed && new_data && parity, out);
  if (rc) return rc;
  const bool pair = old_data != nullptr;
  for (int b = 0; b < batch; ++b)
    for (int i = 0; i < k; ++i)
      if (changed[static_cast<size_t>(b) * k + i] && sizes[b] == 0) return RS_E_NO_DATA;
  for (int b = 0; b < batch; ++b) {
    bool any = false;
    for (int i = 0; i < k; ++i) {
      const size_t at = static_cast<size_t>(b) * k + i;
      if (!changed[at]) continue;
      any = true;
      if (!new_data[at] || (pair && !old_data[at])) return RS_E_ARG;
    }
    for (int j = 0; any && j < m; ++j)
      if (!parity[static_cast<size_t>(b) * m + j]) return RS_E_ARG;
  }
  if (!ctx->device(device)) return RS_E_ARG;
  UpdateTables t;
  if ((rc = table_status(build_update_tables(k, m, batch, sizes, changed, t)))) return rc;
  size_t smax = 0;
  for (int b = 0; b < batch; ++b)
    if (t.has[static_cast<size_t>(b)]) smax = std::max(smax, sizes[b]);
  auto plan = new_plan(device, smax, batch);
  plan->update = std::make_unique<UpdatePlan>();
  UpdatePlan& up = *plan->update;
  up.pair = pair;
  up.cmax = t.cmax;
  up.ntiles = t.map.ntiles;
  up.any_tail = t.map.any_tail;
  plan->fixed_form = RS_ORDER_CONSECUTIVE + kOrderUpdate;
  plan->bytes = pair ? t.bytes_pair : t.bytes_single;
  const size_t stride = static_cast<size_t>(t.cmax) * (pair ? 2 : 1);
  Packer pk;
  plan->status_off = pk.take(sizeof(int) * static_cast<size_t>(batch));
  up.in_off = pk.take(sizeof(void*) * std::max<size_t>(1, static_cast<size_t>(batch) * stride));
  up.pat_off = pk.take(sizeof(uint32_t) * static_cast<size_t>(batch));
  up.nsrc_off = pk.take(sizeof(uint32_t) * std::max<size_t>(1, t.nsrc.size()));
  up.size_off = pk.take(sizeof(uint64_t) * static_cast<size_t>(batch));
  up.tile0_off = pk.take(sizeof(uint32_t) * t.map.tile0.size());
  up.tile_stripe_off = pk.take(sizeof(uint32_t) * std::max<size_t>(1, t.map.tile_stripe.size()));
  for (const UpdateGroup& g : t.groups)
    up.groups.push_back({g.R, pk.take(sizeof(void*) * static_cast<size_t>(batch) * g.R),
                         pk.take(g.arena.size()), static_cast<uint32_t>(g.tab_stride)});
  std::vector<uint8_t> h(pk.off, 0);
  auto put = [&](size_t off, const auto& v) {
    if (!v.empty()) std::memcpy(h.data() + off, v.data(), sizeof(v[0]) * v.size());
  };
  // sources of stripe b: its pattern's changed shards in ascending order, (old, new) for pairs;
  // slots past its source count, and every slot of an unchanged stripe, stay null and unread
  auto* in = reinterpret_cast<const uint8_t**>(h.data() + up.in_off);
  for (int b = 0; b < batch; ++b) {
    if (!t.has[static_cast<size_t>(b)]) continue;
    const std::vector<int>& idx = t.patterns[t.pat[static_cast<size_t>(b)]];
    for (size_t c = 0; c < idx.size(); ++c) {
      const size_t at = static_cast<size_t>(b) * k + idx[c];
      if (pair) {
        in[b * stride + 2 * c] = old_data[at];
        in[b * stride + 2 * c + 1] = new_data[at];
      } else {
        in[b * stride + c] = new_data[at];
      }
    }
  }
  put(up.pat_off, t.pat);
  put(up.nsrc_off, t.nsrc);
  put(up.size_off, t.size);
  put(up.tile0_off, t.map.tile0);
  put(up.tile_stripe_off, t.map.tile_stripe);
  for (size_t gi = 0; gi < t.groups.size(); ++gi) {
    const UpdateGroup& g = t.groups[gi];
    auto* o = reinterpret_cast<uint8_t**>(h.data() + up.groups[gi].out_off);
    for (int b = 0; b < batch; ++b)
      for (int r = 0; r < g.R; ++r)
        o[static_cast<size_t>(b) * g.R + r] =
            t.has[static_cast<size_t>(b)] ? parity[static_cast<size_t>(b) * m + g.row0 + r] : nullptr;
    put(up.groups[gi].arena_off, g.arena);
  }
  if ((rc = upload(plan->dmeta, device, h.data(), h.size()))) return rc;
  *out = plan.release();
  return RS_OK;
}

int rs_plan_create_decode_idx(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                              const uint8_t* expect, const uint8_t* const* input, uint8_t* const* dst,
                              unsigned flags, rs_plan** out) {
  DeviceGuard dg;
  int rc = check_plan_args(ctx, k, m, batch, sizes && expect && input && dst && !(flags & ~RS_DECODE_IDX_STORE),
                           out);
  if (rc) return rc;
  const size_t cells = static_cast<size_t>(batch) * (k + m);
  std::vector<uint8_t> have_in(cells), have_dst(cells);
  for (size_t i = 0; i < cells; ++i) {
    have_in[i] = input[i] != nullptr;
    have_dst[i] = dst[i] != nullptr;
  }
  DecodeIdxTables t;
  if ((rc = decode_idx_status(
           build_decode_idx_tables(k, m, batch, sizes, expect, have_in.data(), have_dst.data(), t))))
    return rc;
  if (!ctx->device(device)) return RS_E_ARG;
  const bool store = (flags & RS_DECODE_IDX_STORE) != 0;
  return finish_decode_plan(device, t, sizes, input, [&](size_t at) { return dst[at]; }, store, false,
                            store ? t.bytes_store : t.bytes_merge, out);
}

int rs_plan_create_decode_check(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                                const uint8_t* expect, const uint8_t* const* input, uint8_t* const* dst,
                                uint8_t* const* check, unsigned flags, rs_plan** out) {
  DeviceGuard dg;
  int rc = check_plan_args(ctx, k, m, batch,
                           sizes && expect && input && dst && check &&
                               !(flags & ~(RS_DECODE_IDX_STORE | RS_DECODE_CHECK_FINAL)),
                           out);
  if (rc) return rc;
  const size_t cells = static_cast<size_t>(batch) * (k + m);
  std::vector<uint8_t> have_in(cells), have_dst(cells), have_chk(cells);
  for (size_t i = 0; i < cells; ++i) {
    have_in[i] = input[i] != nullptr;
    have_dst[i] = dst[i] != nullptr;
    have_chk[i] = check[i] != nullptr;
  }
  const bool store = (flags & RS_DECODE_IDX_STORE) != 0, final = (flags & RS_DECODE_CHECK_FINAL) != 0;
  DecodeCheckTables t;
  if ((rc = decode_idx_status(build_decode_check_tables(k, m, batch, sizes, expect, have_in.data(),
                                                        have_dst.data(), have_chk.data(), final, t))))
    return rc;
  if (!ctx->device(device)) return RS_E_ARG;
  // a non-final plan runs the decode-idx kernels: a check row is an ordinary row there
  return finish_decode_plan(device, t, sizes, input, [&](size_t at) { return check[at] ? check[at] : dst[at]; },
                            store, final, t.bytes[(final ? 2 : 0) + (store ? 1 : 0)], out);
}

int rs_plan_create_decode_repair(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                                 const uint8_t* expect, const uint8_t* const* input, uint8_t* const* dst,
                                 uint8_t* const* check, uint8_t* const* fix, unsigned flags, rs_plan** out) {
  DeviceGuard dg;
  int rc = check_plan_args(ctx, k, m, batch,
                           sizes && expect && input && dst && check && fix && !(flags & ~RS_DECODE_IDX_STORE), out);
  if (rc) return rc;
  const size_t cells = static_cast<size_t>(batch) * (k + m);
  std::vector<uint8_t> have_in(cells), have_dst(cells), have_chk(cells), have_fix(cells);
  for (size_t i = 0; i < cells; ++i) {
    have_in[i] = input[i] != nullptr;
    have_dst[i] = dst[i] != nullptr;
    have_chk[i] = check[i] != nullptr;
    have_fix[i] = fix[i] != nullptr;
  }
  DecodeRepairTables t;
  switch (build_decode_repair_tables(k, m, batch, sizes, expect, have_in.data(), have_dst.data(), have_chk.data(),
                                     have_fix.data(), t)) {
    case DecodeRepairError::kOk: break;
    case DecodeRepairError::kArg: return RS_E_ARG;
    case DecodeRepairError::kTooFewShards: return RS_E_TOO_FEW_SHARDS;
    case DecodeRepairError::kUnsupported: return RS_E_UNSUPPORTED;
    case DecodeRepairError::kNoData: return RS_E_NO_DATA;
    case DecodeRepairError::kTooManyTiles: return RS_E_ARG;  // a grid past 2^31 - 1 tiles
    case DecodeRepairError::kSingular: return RS_E_SINGULAR;
  }
  if (!ctx->device(device)) return RS_E_ARG;
  const bool store = (flags & RS_DECODE_IDX_STORE) != 0;
  // the final decode-check figure: the few repaired bytes are not counted
  return finish_decode_plan(device, t.c, sizes, input, [&](size_t at) { return check[at] ? check[at] : dst[at]; },
                            store, true, t.c.bytes[2 + (store ? 1 : 0)], out, &t, fix);
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

// The counts a locate or decode-repair plan's launches have added since the last read, then cleared (as
// rs_plan_stripe_status does with the flags): a plan launched twice before a read reports
// every count doubled.
int rs_plan_blame(rs_plan* plan, void* stream, uint64_t* counts) {
  DeviceGuard dg;
  if (!plan || !counts) return RS_E_ARG;
  const bool locate = plan->mixed && plan->mixed->kind == PlanKind::kLocate;
  const bool repair = plan->update && plan->update->repair;
  if (!locate && !repair) return RS_E_ARG;
  HIPCHK(hipSetDevice(plan->device));
  auto s = static_cast<hipStream_t>(stream);
  const size_t off = locate ? plan->mixed->counts_off : plan->update->counts_off;
  const int n = locate ? plan->mixed->t.k + plan->mixed->t.m : plan->update->k + plan->update->m;
  auto* c = static_cast<uint8_t*>(plan->dmeta.p) + off;
  const size_t bytes = sizeof(uint64_t) * static_cast<size_t>(plan->batch) * (n + 1);
  HIPCHK(hipMemcpyAsync(counts, c, bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemsetAsync(c, 0, bytes, s));
  HIPCHK(hipStreamSynchronize(s));
  return RS_OK;
}

uint64_t rs_plan_bytes(const rs_plan* plan) { return plan ? plan->bytes : 0; }

int rs_plan_groups(const rs_plan* plan) { return plan ? static_cast<int>(plan_groups(*plan)) : 0; }

// ---- feed objects -----------------------------------------------------------

int rs_feed_create(rs_ctx* ctx, int device, int k, int m, size_t S, const uint8_t* expect, uint8_t* const* dst,
                   uint8_t* const* check, rs_feed** out) {
  DeviceGuard dg;
  if (const int rc = check_profile(k, m)) return rc;
  if (!ctx || !expect || !dst || !check || !out) return RS_E_ARG;
  *out = nullptr;
  const size_t n = static_cast<size_t>(k + m);
  std::vector<uint8_t> have_dst(n), have_chk(n);
  for (size_t i = 0; i < n; ++i) {
    have_dst[i] = dst[i] != nullptr;
    have_chk[i] = check[i] != nullptr;
  }
  auto feed = std::make_unique<rs_feed>();
  switch (build_feed_tables(k, m, S, expect, have_dst.data(), have_chk.data(), feed->t)) {
    case FeedError::kOk: break;
    case FeedError::kArg: return RS_E_ARG;
    case FeedError::kTooFewShards: return RS_E_TOO_FEW_SHARDS;
    case FeedError::kUnsupported: return RS_E_UNSUPPORTED;
    case FeedError::kNoData: return RS_E_NO_DATA;
    case FeedError::kSingular: return RS_E_SINGULAR;
  }
  if (!ctx->device(device)) return RS_E_ARG;
  feed->device = device;
  feed->S = S;
  for (int i : feed->t.rows) feed->rows.push_back(check[i] ? check[i] : dst[i]);
  constexpr size_t kRowTabBytes = kFeedMaxRows * sizeof(uint8_t*);
  std::vector<uint8_t> h(kRowTabBytes + feed->t.arena.size() * sizeof(uint32_t), 0);
  if (!feed->rows.empty()) {
    std::memcpy(h.data(), feed->rows.data(), feed->rows.size() * sizeof(uint8_t*));
    std::memcpy(h.data() + kRowTabBytes, feed->t.arena.data(), feed->t.arena.size() * sizeof(uint32_t));
  }
  if (const int rc = upload(feed->dmeta, device, h.data(), h.size())) return rc;
  *out = feed.release();
  return RS_OK;
}

int rs_feed_launch(rs_feed* feed, int idx, const uint8_t* src, unsigned flags, void* stream) {
  DeviceGuard dg;
  if (!feed || !src || (flags & ~RS_DECODE_IDX_STORE)) return RS_E_ARG;
  const int pos = feed->t.position(idx);
  if (pos < 0) return RS_E_ARG;
  if (feed->t.R() == 0) return RS_OK;  // no row: nothing to enqueue
  HIPCHK(hipSetDevice(feed->device));
  auto* d = static_cast<uint8_t*>(feed->dmeta.p);
  FeedArgs x{};
  x.src = src;
  x.tabs = reinterpret_cast<const uint32_t*>(d + kFeedMaxRows * sizeof(uint8_t*)) +
           static_cast<size_t>(pos) * feed->t.block_words();
  x.row_tab = reinterpret_cast<uint8_t* const*>(d);
  x.rows = feed->rows.data();
  x.S = feed->S;
  x.R = feed->t.R();
  HIPCHK(launch_feed(x, (flags & RS_DECODE_IDX_STORE) != 0, static_cast<hipStream_t>(stream)));
  return RS_OK;
}

void rs_feed_destroy(rs_feed* feed) {
  DeviceGuard dg;
  delete feed;
}

// ---- absorb objects ---------------------------------------------------------

int rs_absorb_create(rs_ctx* ctx, int device, int k, int m, size_t S, uint8_t* const* rows, rs_absorb** out) {
  DeviceGuard dg;
  if (const int rc = check_profile(k, m)) return rc;
  if (!ctx || !rows || !out) return RS_E_ARG;
  *out = nullptr;
  if (m <= kAbsorbMaxRows)
    for (int j = 0; j < m; ++j)
      if (!rows[j]) return RS_E_ARG;
  auto ab = std::make_unique<rs_absorb>();
  switch (build_absorb_tables(k, m, S, ab->t)) {
    case AbsorbError::kOk: break;
    case AbsorbError::kUnsupported: return RS_E_UNSUPPORTED;
    case AbsorbError::kNoData: return RS_E_NO_DATA;
    case AbsorbError::kSingular: return RS_E_SINGULAR;
  }
  if (!ctx->device(device)) return RS_E_ARG;
  ab->device = device;
  ab->S = S;
  ab->rows.assign(rows, rows + m);
  ab->scratch.reserve(kAbsorbMaxIntervals);
  constexpr size_t kRowTabBytes = kAbsorbMaxRows * sizeof(uint8_t*);
  std::vector<uint8_t> h(kRowTabBytes + ab->t.arena.size() * sizeof(uint32_t), 0);
  std::memcpy(h.data(), ab->rows.data(), ab->rows.size() * sizeof(uint8_t*));
  std::memcpy(h.data() + kRowTabBytes, ab->t.arena.data(), ab->t.arena.size() * sizeof(uint32_t));
  if (const int rc = upload(ab->dmeta, device, h.data(), h.size())) return rc;
  *out = ab.release();
  return RS_OK;
}

int rs_absorb_launch(rs_absorb* ab, uint64_t off, uint64_t len, const uint8_t* src, void* stream) {
  DeviceGuard dg;
  if (!ab || !src) return RS_E_ARG;
  AbsorbArgs x{};
  {
    // the plan's scratch vector is the object's: launches of one object may come from any thread
    std::lock_guard<std::mutex> g(ab->mu);
    if (!absorb_plan(ab->t.k, ab->S, off, len, x.plan, ab->scratch)) return RS_E_ARG;
  }
  HIPCHK(hipSetDevice(ab->device));
  auto* d = static_cast<uint8_t*>(ab->dmeta.p);
  x.src = src;
  x.tabs = reinterpret_cast<const uint32_t*>(d + kAbsorbMaxRows * sizeof(uint8_t*));
  x.row_tab = reinterpret_cast<uint8_t* const*>(d);
  x.rows = ab->rows.data();
  x.S = ab->S;
  x.off = off;
  x.len = len;
  x.K = ab->t.k;
  x.R = ab->t.m;
  HIPCHK(launch_absorb(x, static_cast<hipStream_t>(stream)));
  return RS_OK;
}

void rs_absorb_destroy(rs_absorb* ab) {
  DeviceGuard dg;
  delete ab;
}

// ---- one-shot device calls ------------------------------------------------------------------------

int rs_encode_dev(rs_ctx* ctx, int device, int k, int m, size_t S, int batch,
                  uint8_t* const* shards, void* stream) {
  return one_shot([&](rs_plan** p) { return rs_plan_create(ctx, device, k, m, S, batch, nullptr, shards, p); },
                  stream);
}

int rs_decode_dev(rs_ctx* ctx, int device, int k, int m, size_t S, int batch,
                  const uint8_t* present, uint8_t* const* shards, void* stream) {
  if (!present) return RS_E_ARG;
  return one_shot([&](rs_plan** p) { return rs_plan_create(ctx, device, k, m, S, batch, present, shards, p); },
                  stream);
}

int rs_decode_dev_mixed(rs_ctx* ctx, int device, int k, int m, size_t S, int batch,
                        const uint8_t* present, uint8_t* const* shards, void* stream) {
  if (!present) return RS_E_ARG;
  return one_shot(
      [&](rs_plan** p) { return rs_plan_create_mixed(ctx, device, k, m, S, batch, present, shards, p); }, stream);
}

int rs_decode_dev_ragged(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                         const uint8_t* present, uint8_t* const* shards, void* stream) {
  return one_shot(
      [&](rs_plan** p) { return rs_plan_create_ragged(ctx, device, k, m, batch, sizes, present, shards, p); },
      stream);
}

int rs_decode_dev_required(rs_ctx* ctx, int device, int k, int m, int batch, const size_t* sizes,
                           const uint8_t* present, const uint8_t* required,
                           uint8_t* const* shards, void* stream) {
  return one_shot(
      [&](rs_plan** p) {
        return rs_plan_create_required(ctx, device, k, m, batch, sizes, present, required, shards, p);
      },
      stream);
}

}  // extern "C"
