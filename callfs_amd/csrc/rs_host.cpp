// The host-memory path of the C ABI (include/callfs_rs.h): the per-object calls
// (Codec.Encode / Decode ends, Encode, Reconstruct, Verify), the batch calls and the router
// that sends a batch call's runnable stripes through the pipelines (run_batch).
//
// The control flow and error precedence follow codec.go:21-78 and the upstream
// reedsolomon methods it calls (Split/Encode at :31/:36, Reconstruct at :55, Verify at
// :59). Stripes of one table set and shard size go through host_uniform.hpp, a batch of mixed
// sizes or erasures through host_ragged.hpp; what a call admits, how a batch is routed and
// Split's shape are the HIP-free host_path.hpp and codec_batch.hpp. Every reconstruct, with a
// wanted set (ReconstructSome / ReconstructData) or without, is admitted into the same kShard*
// flag rows and takes the same path from there. Locate (which shard is corrupt, DESIGN.md
// §5.12) runs through host_locate.hpp, and the heal calls compose it with the reconstructs;
// correct (repair in place from the syndromes, §5.13) through host_correct.hpp. The ragged,
// update and locate routes are jobs of one chunk pipeline (host_chunks.hpp, §7.5). The checksummed
// codec batches (§7.7) are the codec batches with a SumsCall handed to the ragged pipeline; what
// they hash where, and a decode's follow-up run, are the HIP-free sums_table.hpp / sums_host.hpp.
#include "codec_batch.hpp"
#include "host_correct.hpp"
#include "host_locate.hpp"
#include "host_ragged.hpp"
#include "host_uniform.hpp"
#include "host_decode_idx.hpp"
#include "host_decode_repair.hpp"
#include "host_update.hpp"
#include "overwrite_plan.hpp"

using namespace callfs;

namespace {

// The encode tables of RS(k, m): every data shard present, the parity rows computed.
std::shared_ptr<const Tables> encode_tables(rs_ctx* ctx, int k, int m) {
  uint8_t present[256];
  for (int i = 0; i < k + m; ++i) present[i] = i < k;
  return ctx->cache.get(k, m, present, false);
}

// Shared by rs_reconstruct / rs_codec_decode. verify=true fuses upstream Verify. `joined`
// (nullable) asks for decode's join of original_size bytes into `out` on the way through
// the pipeline and tells whether the pipeline ran and wrote it. wanted (nullable, k+m flags):
// the missing shards to rebuild (rs_reconstruct_some, rs_codec_decode_data); the others are
// neither written nor read.
int reconstruct_host(rs_ctx* ctx, int k, int m, uint8_t* const* shards, size_t* lens,
                     bool verify, uint8_t* out = nullptr, size_t original_size = 0,
                     bool* joined = nullptr, const uint8_t* wanted = nullptr) {
  uint8_t flags[256], present[256], want[256];
  const StripeAdmission a = admit_stripe(k + m, k, shards, lens, wanted, verify, flags);
  if (!a.run) return a.status;
  shard_flags_split(flags, static_cast<size_t>(k + m), present, want);
  auto t = ctx->cache.get(k, m, present, verify, want);
  if (!t) return RS_E_SINGULAR;
  if (t->groups.empty()) return RS_OK;
  const Join join = decode_join(k, a.S, out, original_size);
  const int rc = run_host1(ctx, t, a.S, [&](int i) { return shards[i]; },
                           [&](int i) { return shards[i]; }, joined ? &join : nullptr);
  if (rc == RS_OK || rc == RS_E_CORRUPT) {
    for (int i : t->missing) lens[i] = a.S;
    if (joined) *joined = true;
  }
  return rc;
}

int first_error(const int* status, int batch) {
  for (int b = 0; b < batch; ++b)
    if (status[b]) return status[b];
  return RS_OK;
}

// A batch call's tables: whether they compare the present shards beyond the first k, and
// whether a ragged run drops the compared rows (a reconstruct without verify).
struct BatchMode {
  bool verify;
  bool by_missing;
};

// The runnable stripes of a batch call (`groups`) on the route batch_route (host_path.hpp)
// chooses: one ragged pipeline, or one uniform pipeline per (S, flag row) group. S, present (n
// kShard* flags each, host_path.hpp), joins (nullable) and flags are indexed by the call's
// stripes; in(b, i) / out(b, i) give stripe b's shard i. flags[b] = 1 where stripe b's compared
// rows mismatched.
// One call is counted: by run_ragged, or with the first group that runs (tables without
// launch groups run nothing). Returns RS_OK or the error that ended the call.
// sums (nullable): a checksummed codec batch, indexed by the call's stripes
// like the rest. It takes the ragged pipeline whatever its groups are, and there the staged
// transport.
template <class InF, class OutF>
int run_batch(rs_ctx* ctx, int k, int m, BatchMode mode, const BatchGroups& groups,
              const size_t* S, const uint8_t* present, const Join* joins, InF in, OutF out,
              int* flags, SumsCall* sums = nullptr) {
  const size_t n = static_cast<size_t>(k + m);
  BatchRoute route = batch_route(groups, ragged_batch() || sums);
  if (sums && !route.ragged && !groups.stripes.empty()) {
    route.ragged = true;
    route.ids = groups.stripes;
    std::sort(route.ids.begin(), route.ids.end());
  }
  if (route.ragged) {
    const std::vector<int>& ids = route.ids;
    if (sums) sums->obj = ids.data();
    std::vector<size_t> Sj(ids.size());
    std::vector<uint8_t> pres(ids.size() * n);
    std::vector<Join> jj;
    for (size_t j = 0; j < ids.size(); ++j) {
      const size_t b = static_cast<size_t>(ids[j]);
      Sj[j] = S[b];
      std::memcpy(&pres[j * n], &present[b * n], n);
      if (joins) jj.push_back(joins[b]);
    }
    std::vector<int> fj(ids.size(), 0);
    const int rc = run_ragged(ctx, k, m, mode.by_missing, Sj, pres,
                              [&](int j, int i) { return in(ids[j], i); },
                              [&](int j, int i) { return out(ids[j], i); }, fj.data(),
                              joins ? jj.data() : nullptr, sums);
    for (size_t j = 0; j < ids.size(); ++j) flags[ids[j]] = fj[j];
    return rc;
  }
  bool first = true;
  for (const auto* kv : route.groups) {
    const std::vector<int>& ids = kv->second;
    uint8_t pres[256], want[256];
    shard_flags_split(BatchGroups::present(kv->first), n, pres, want);
    auto t = ctx->cache.get(k, m, pres, mode.verify, want);
    if (!t) return RS_E_SINGULAR;
    if (t->groups.empty()) continue;
    std::vector<Join> jj;
    for (int b : ids)
      if (joins) jj.push_back(joins[b]);
    std::vector<int> fj(ids.size(), 0);
    const int rc = run_host(ctx, t, BatchGroups::shard_size(kv->first), static_cast<int>(ids.size()),
                            [&](int b, int i) { return in(ids[b], i); },
                            [&](int b, int i) { return out(ids[b], i); }, fj.data(),
                            joins ? jj.data() : nullptr, first);
    first = false;
    if (rc != RS_OK && rc != RS_E_CORRUPT) return rc;
    for (size_t j = 0; j < ids.size(); ++j) flags[ids[j]] = fj[j];
  }
  return RS_OK;
}

// Shared by rs_reconstruct_batch / rs_codec_decode_batch, as reconstruct_host is by the
// single calls. out and original_sizes (both or neither) ask for decode's join per object.
// required (nullable, batch * n flags) or data_only (the data shards) name the missing shards
// to rebuild: the others are neither written nor read, a stripe without a row reaches no
// device, and decode's join of such a stripe is a plain copy of its data shards.
// expected and bad (both or neither; batch * n digests and flags): rs_codec_decode_batch_sums.
// The admitted objects run with every present shard taken as good and their shards hashed on
// the way; nothing of an object with a mismatch is delivered, and those objects then run
// again, in one plain call of this function, with their bad shards' lengths zero.
int reconstruct_batch_host(rs_ctx* ctx, int k, int m, int batch, uint8_t* const* shards,
                           size_t* lens, bool verify, uint8_t* const* out,
                           const int64_t* original_sizes, int* status,
                           const uint8_t* required = nullptr, bool data_only = false,
                           const uint8_t* expected = nullptr, uint8_t* bad = nullptr) {
  const size_t n = static_cast<size_t>(k + m), B = static_cast<size_t>(batch);
  std::vector<uint8_t> present(B * n, 0);
  std::vector<size_t> S(B, 0);  // nonzero for the stripes that run
  std::vector<Join> joins(out ? B : 0, Join{nullptr, 0, 0, k});
  std::vector<uint8_t> data_flags(data_only ? n : 0, 0);
  for (int i = 0; data_only && i < k; ++i) data_flags[static_cast<size_t>(i)] = 1;
  std::vector<CopyPool::Seg> copies;  // the joins of stripes without a row
  BatchGroups groups;
  for (size_t b = 0; b < B; ++b) {
    const StripeAdmission a =
        admit_stripe(k + m, k, shards + b * n, lens + b * n,
                     data_only ? data_flags.data() : required ? required + b * n : nullptr, verify,
                     &present[b * n]);
    status[b] = a.status;
    if (!a.run && out && a.status == RS_OK) {
      // admitted, nothing to compute: every data shard is present (data_only)
      if (original_sizes[b] < 0 || (original_sizes[b] != 0 && !out[b])) {
        status[b] = RS_E_ARG;
        continue;
      }
      const Join j = decode_join(k, a.S, out[b], static_cast<size_t>(original_sizes[b]));
      for (int i = 0; i < k; ++i) {
        const auto js = join_span(&j, i, 0, a.S);
        if (js.first) copies.push_back({js.first, shards[b * n + static_cast<size_t>(i)], js.second});
      }
      if (static_cast<uint64_t>(a.S) * k < static_cast<uint64_t>(original_sizes[b]))
        status[b] = RS_E_INSUFFICIENT;
      continue;
    }
    if (!a.run) continue;
    if (out) {
      // a runnable object's own arguments: the same RS_E_ARG as a NULL shard
      if (original_sizes[b] < 0 || (original_sizes[b] != 0 && !out[b])) {
        status[b] = RS_E_ARG;
        continue;
      }
      joins[b] = decode_join(k, a.S, out[b], static_cast<size_t>(original_sizes[b]));
    }
    S[b] = a.S;
    groups.add(a.S, &present[b * n], k + m, static_cast<int>(b));
  }
  std::vector<int> flags(B, 0);
  auto shard = [&](int b, int i) { return shards[static_cast<size_t>(b) * n + i]; };
  if (!copies.empty()) ctx->pool.run(copies);
  SumsCall sums;
  sums.mode = SumsMode::kCheck;
  sums.n = k + m;
  sums.expected = expected;
  sums.bad = bad;
  if (bad) std::memset(bad, 0, B * n);
  int rc = run_batch(ctx, k, m, BatchMode{verify, !verify}, groups, S.data(), present.data(),
                     out ? joins.data() : nullptr, shard, shard, flags.data(), bad ? &sums : nullptr);
  if (rc) return rc;
  if (bad) {
    SumsRerun again(k + m, batch, S.data(), bad, shards, lens, out, original_sizes);
    if (again.count()) {
      rc = reconstruct_batch_host(ctx, k, m, again.count(), again.shards.data(), again.lens.data(),
                                  verify, again.out.data(), again.sizes.data(), again.status.data());
      if (rc && rc != first_error(again.status.data(), again.count())) return rc;  // call-level
      again.finish(k + m, lens, status, [](int st) {
        return st == RS_OK || st == RS_E_CORRUPT || st == RS_E_INSUFFICIENT;
      });
      for (int b : again.objs) S[static_cast<size_t>(b)] = 0;  // done
    }
  }
  for (size_t b = 0; b < B; ++b) {
    if (!S[b]) continue;
    for (size_t i = 0; i < n; ++i)
      if (!present[b * n + i]) lens[b * n + i] = S[b];  // the rebuilt shards
    if (flags[b])
      status[b] = RS_E_CORRUPT;
    else if (out && static_cast<uint64_t>(S[b]) * k < static_cast<uint64_t>(original_sizes[b]))
      status[b] = RS_E_INSUFFICIENT;
  }
  return first_error(status, batch);
}

// Shared by rs_update, rs_encode_idx, rs_update_batch and rs_codec_overwrite: stripe b's shard i
// changed where new_data[b*k + i] is non-NULL; old_data null (the array) is EncodeIdx mode.
// status[b]: RS_OK, RS_E_NO_DATA (a change in a stripe of size 0) or RS_E_ARG (a changed shard
// without its old bytes, a NULL parity pointer); the other stripes run. Stripes without a
// change are RS_OK and reach no device.
int update_batch_host(rs_ctx* ctx, int k, int m, int batch, const size_t* sizes,
                      const uint8_t* const* old_data, const uint8_t* const* new_data,
                      uint8_t* const* parity, int* status) {
  const size_t B = static_cast<size_t>(batch), K = static_cast<size_t>(k);
  std::vector<uint8_t> changed(B * K, 0);
  std::vector<int> ids;
  for (size_t b = 0; b < B; ++b) {
    status[b] = RS_OK;
    bool any = false, bad = false;
    for (size_t i = 0; i < K; ++i) {
      if (!new_data[b * K + i]) continue;
      any = true;
      changed[b * K + i] = 1;
      bad |= old_data && !old_data[b * K + i];
    }
    if (!any) continue;
    for (int j = 0; j < m; ++j) bad |= !parity[b * static_cast<size_t>(m) + j];
    if (sizes[b] == 0) status[b] = RS_E_NO_DATA;
    else if (bad) status[b] = RS_E_ARG;
    else ids.push_back(static_cast<int>(b));
  }
  return run_update(ctx, k, m, old_data != nullptr, ids, sizes, changed.data(),
                    [&](int b, int i) { return old_data[static_cast<size_t>(b) * K + i]; },
                    [&](int b, int i) { return new_data[static_cast<size_t>(b) * K + i]; },
                    [&](int b, int j) { return parity[static_cast<size_t>(b) * m + j]; });
}

// rs_codec_decode, and with data_only rs_codec_decode_data: upstream ReconstructData in
// Reconstruct's place, so missing parity stays missing.
int codec_decode(rs_ctx* ctx, int k, int m, uint8_t* const* shards, size_t* lens, uint8_t* out,
                 int64_t original_size, bool data_only) {
  DeviceGuard dg;
  // codec.go:46-48 profile, :50 New, :55 Reconstruct, :59-65 Verify, :67-77 join/trim
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || !shards || !lens || original_size < 0 || (original_size && !out)) return RS_E_ARG;
  bool joined = false;
  uint8_t data_flags[256] = {0};
  for (int i = 0; i < k; ++i) data_flags[i] = 1;
  rc = reconstruct_host(ctx, k, m, shards, lens, true, out, static_cast<size_t>(original_size),
                        &joined, data_only ? data_flags : nullptr);
  if (rc) return rc;
  const size_t S = lens[0];
  if (static_cast<uint64_t>(S) * k < static_cast<uint64_t>(original_size))
    return RS_E_INSUFFICIENT;
  if (joined) return RS_OK;  // joined on the way through the pipeline
  size_t left = static_cast<size_t>(original_size);
  std::vector<CopyPool::Seg> segs;
  for (int i = 0; i < k && left; ++i) {
    const size_t c = std::min(S, left);
    segs.push_back({out + S * i, shards[i], c});
    left -= c;
  }
  ctx->pool.run(segs);
  return RS_OK;
}

// Shared by rs_locate, rs_locate_batch and the heal calls: admission as a reconstruct with
// verify that wants nothing (so a stripe of exactly k present shards is RS_OK with zero counts
// and no device work), then the locate pipeline over the stripes with a compared shard.
// counts: batch * (k + m + 1), written for every stripe; status[b] = RS_E_CORRUPT where a
// syndrome of stripe b was nonzero. max_errors 1 or 2 (checked by the exported calls): 2 locates
// with pair tables, and a column blamed on two shards counts in both.
int locate_batch_host(rs_ctx* ctx, int k, int m, int max_errors, int batch, const uint8_t* const* shards,
                      const size_t* lens, uint64_t* counts, int* status) {
  const size_t n = static_cast<size_t>(k + m), B = static_cast<size_t>(batch);
  std::fill(counts, counts + B * (n + 1), 0);
  std::vector<uint8_t> present(B * n, 0), none(n, 0), row(n, 0);
  std::vector<size_t> S(B, 0);
  std::vector<int> ids;
  for (size_t b = 0; b < B; ++b) {
    const StripeAdmission a = admit_stripe(k + m, k, shards + b * n, lens + b * n, none.data(), true, row.data());
    status[b] = a.status;
    if (!a.run) continue;
    S[b] = a.S;
    for (size_t i = 0; i < n; ++i) present[b * n + i] = row[i] == kShardPresent;
    ids.push_back(static_cast<int>(b));
  }
  std::vector<int> flags(B, 0);
  const int rc = run_locate(ctx, k, m, max_errors, ids, S.data(), present.data(),
                            [&](int b, int i) { return shards[static_cast<size_t>(b) * n + i]; }, counts,
                            flags.data());
  if (rc) return rc;
  for (size_t b = 0; b < B; ++b)
    if (flags[b]) status[b] = RS_E_CORRUPT;
  return RS_OK;
}

// rs_heal_batch's body (and, for one stripe, rs_codec_decode_heal's): reconstruct + verify;
// the corrupt stripes are located over their original presence; where every mismatching column
// is explained by a set B of shards and a compared row is left without them, B and the
// originally missing shards (rebuilt from corrupt inputs the first time) are rebuilt and the
// rest verified again. Present shards outside B are never written.
int heal_batch_host(rs_ctx* ctx, int k, int m, int max_errors, int batch, uint8_t* const* shards,
                    size_t* lens, uint8_t* healed, int* status) {
  const size_t n = static_cast<size_t>(k + m), B = static_cast<size_t>(batch);
  std::fill(healed, healed + B * n, 0);
  const std::vector<size_t> lens0(lens, lens + B * n);
  int rc = reconstruct_batch_host(ctx, k, m, batch, shards, lens, true, nullptr, nullptr, status);
  if (rc != RS_OK && rc != first_error(status, batch)) return rc;  // call-level
  std::vector<int> bad;
  for (size_t b = 0; b < B; ++b)
    if (status[b] == RS_E_CORRUPT) bad.push_back(static_cast<int>(b));
  if (bad.empty()) return rc;
  // (b) locate, over the original presence
  const size_t nb = bad.size();
  std::vector<const uint8_t*> sh1(nb * n);
  std::vector<size_t> ln1(nb * n);
  for (size_t j = 0; j < nb; ++j)
    for (size_t i = 0; i < n; ++i) {
      sh1[j * n + i] = shards[static_cast<size_t>(bad[j]) * n + i];
      ln1[j * n + i] = lens0[static_cast<size_t>(bad[j]) * n + i];
    }
  std::vector<uint64_t> counts(nb * (n + 1));
  std::vector<int> st1(nb, RS_OK);
  if ((rc = locate_batch_host(ctx, k, m, max_errors, static_cast<int>(nb), sh1.data(), ln1.data(), counts.data(),
                              st1.data())))
    return rc;
  // (c) the stripes whose blamed set leaves a row to confirm with
  std::vector<int> cand;  // indices into bad
  std::vector<uint8_t*> sh2;
  std::vector<size_t> ln2;
  for (size_t j = 0; j < nb; ++j) {
    const uint64_t* c = &counts[j * (n + 1)];
    size_t blamed = 0, np = 0;
    for (size_t i = 0; i < n; ++i) {
      blamed += c[i] != 0;
      np += ln1[j * n + i] != 0;
    }
    if (c[n] != 0 || blamed == 0 || np - blamed < static_cast<size_t>(k) + 1) continue;
    cand.push_back(static_cast<int>(j));
    for (size_t i = 0; i < n; ++i) {
      sh2.push_back(shards[static_cast<size_t>(bad[j]) * n + i]);
      ln2.push_back(c[i] != 0 ? 0 : ln1[j * n + i]);
    }
  }
  if (!cand.empty()) {
    std::vector<int> st2(cand.size(), RS_OK);
    rc = reconstruct_batch_host(ctx, k, m, static_cast<int>(cand.size()), sh2.data(), ln2.data(), true,
                                nullptr, nullptr, st2.data());
    if (rc != RS_OK && rc != first_error(st2.data(), static_cast<int>(cand.size()))) return rc;
    for (size_t q = 0; q < cand.size(); ++q) {
      if (st2[q] != RS_OK) continue;
      const size_t j = static_cast<size_t>(cand[q]), b = static_cast<size_t>(bad[j]);
      status[b] = RS_OK;
      for (size_t i = 0; i < n; ++i) healed[b * n + i] = counts[j * (n + 1) + i] != 0;
    }
  }
  return first_error(status, batch);
}

}  // namespace

// ---- exported: per-object calls ---------------------------------------------------------

extern "C" {

int rs_encode(rs_ctx* ctx, int k, int m, size_t S, const uint8_t* const* data,
              uint8_t* const* parity) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || !data || !parity) return RS_E_ARG;
  if (S == 0) return RS_E_NO_DATA;  // upstream Encode: checkShards -> ErrShardNoData
  auto t = encode_tables(ctx, k, m);
  if (!t) return RS_E_SINGULAR;
  return run_host1(ctx, t, S, [&](int i) { return data[i]; },
                  [&](int i) { return parity[i - k]; });
}

int rs_codec_encode(rs_ctx* ctx, int k, int m, const uint8_t* data, size_t len,
                    uint8_t* shards_out, size_t out_cap, size_t* shard_size) {
  DeviceGuard dg;
  // codec.go:22-24 profile check, :26 New, :31 Split, :36 Encode. Upstream New accepts
  // k+m > 256 (Leopard), so an empty object fails in Split before the profile is
  // found unsupported here.
  if (k < 1 || m < 1) return RS_E_INVALID_PROFILE;
  if (!ctx || !shard_size || (len && (!data || !shards_out))) return RS_E_ARG;
  if (len == 0) return RS_E_SHORT_DATA;
  int rc = check_profile(k, m);
  if (rc) return rc;
  SplitPlan plan = split_plan(k, len);
  const size_t S = plan.S;
  if (out_cap / static_cast<size_t>(k + m) < S) return RS_E_ARG;
  auto t = encode_tables(ctx, k, m);
  if (!t) return RS_E_SINGULAR;
  *shard_size = S;
  // In place (or overlapping, moved first) every row is read from shards_out. Disjoint
  // buffers: the full data shards are staged straight from `data`, and the staging copies tee
  // them into shards_out (no separate object-sized copy).
  split_prepare(plan, k + m, data, shards_out);
  const Join tee = split_tee(plan, shards_out);
  return run_host1(ctx, t, S, [&](int i) { return split_row(plan, data, shards_out, i); },
                   [&](int i) { return shards_out + S * i; }, &tee);
}

int rs_reconstruct(rs_ctx* ctx, int k, int m, uint8_t* const* shards, size_t* lens) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || !shards || !lens) return RS_E_ARG;
  return reconstruct_host(ctx, k, m, shards, lens, false);
}

int rs_reconstruct_some(rs_ctx* ctx, int k, int m, uint8_t* const* shards, size_t* lens,
                        const uint8_t* required) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || !shards || !lens) return RS_E_ARG;
  return reconstruct_host(ctx, k, m, shards, lens, false, nullptr, 0, nullptr, required);
}

int rs_verify(rs_ctx* ctx, int k, int m, const uint8_t* const* shards, const size_t* lens,
              int* ok) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || !shards || !lens || !ok) return RS_E_ARG;
  const int n = k + m;
  size_t S = 0;
  int np = 0;
  if ((rc = check_lens(n, lens, false, &S, &np))) return rc;
  uint8_t present[256];
  for (int i = 0; i < n; ++i) present[i] = 1;
  auto t = ctx->cache.get(k, m, present, true);
  if (!t) return RS_E_SINGULAR;
  rc = run_host1(ctx, t, S, [&](int i) { return shards[i]; },
                 [&](int) { return static_cast<uint8_t*>(nullptr); });
  if (rc == RS_OK || rc == RS_E_CORRUPT) {
    *ok = rc == RS_OK;
    return RS_OK;
  }
  return rc;
}

int rs_codec_decode(rs_ctx* ctx, int k, int m, uint8_t* const* shards, size_t* lens,
                    uint8_t* out, int64_t original_size) {
  return codec_decode(ctx, k, m, shards, lens, out, original_size, false);
}

int rs_codec_decode_data(rs_ctx* ctx, int k, int m, uint8_t* const* shards, size_t* lens,
                         uint8_t* out, int64_t original_size) {
  return codec_decode(ctx, k, m, shards, lens, out, original_size, true);
}

// ---- exported: locate and heal ----------------------------------------

// max_errors of the _ex calls: below 1 is an argument error (with the NULL and count checks),
// above 2 is not built; both before any device work.
static int check_max_errors(int max_errors) { return max_errors > 2 ? RS_E_UNSUPPORTED : RS_OK; }

int rs_locate_batch_ex(rs_ctx* ctx, int k, int m, int batch, const uint8_t* const* shards,
                       const size_t* lens, uint64_t* counts, int* status, int max_errors) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || batch < 0 || max_errors < 1 || (batch && (!shards || !lens || !counts || !status))) return RS_E_ARG;
  if ((rc = check_max_errors(max_errors))) return rc;
  if ((rc = locate_batch_host(ctx, k, m, max_errors, batch, shards, lens, counts, status))) return rc;
  return first_error(status, batch);
}

int rs_locate_batch(rs_ctx* ctx, int k, int m, int batch, const uint8_t* const* shards,
                    const size_t* lens, uint64_t* counts, int* status) {
  return rs_locate_batch_ex(ctx, k, m, batch, shards, lens, counts, status, 1);
}

int rs_locate_ex(rs_ctx* ctx, int k, int m, const uint8_t* const* shards, const size_t* lens,
                 uint64_t* counts, int max_errors) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || !shards || !lens || !counts || max_errors < 1) return RS_E_ARG;
  if ((rc = check_max_errors(max_errors))) return rc;
  int status = RS_OK;
  if ((rc = locate_batch_host(ctx, k, m, max_errors, 1, shards, lens, counts, &status))) return rc;
  return status;
}

int rs_locate(rs_ctx* ctx, int k, int m, const uint8_t* const* shards, const size_t* lens,
              uint64_t* counts) {
  return rs_locate_ex(ctx, k, m, shards, lens, counts, 1);
}

int rs_heal_batch_ex(rs_ctx* ctx, int k, int m, int batch, uint8_t* const* shards, size_t* lens,
                     uint8_t* healed, int* status, int max_errors) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || batch < 0 || max_errors < 1 || (batch && (!shards || !lens || !healed || !status))) return RS_E_ARG;
  if ((rc = check_max_errors(max_errors))) return rc;
  if (batch == 0) return RS_OK;
  return heal_batch_host(ctx, k, m, max_errors, batch, shards, lens, healed, status);
}

int rs_heal_batch(rs_ctx* ctx, int k, int m, int batch, uint8_t* const* shards, size_t* lens,
                  uint8_t* healed, int* status) {
  return rs_heal_batch_ex(ctx, k, m, batch, shards, lens, healed, status, 1);
}

int rs_codec_decode_heal_ex(rs_ctx* ctx, int k, int m, uint8_t* const* shards, size_t* lens,
                            uint8_t* out, int64_t original_size, uint8_t* healed, int max_errors) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || !shards || !lens || !healed || original_size < 0 || (original_size && !out) || max_errors < 1)
    return RS_E_ARG;
  if ((rc = check_max_errors(max_errors))) return rc;
  const size_t n = static_cast<size_t>(k + m);
  std::fill(healed, healed + n, 0);
  const std::vector<size_t> lens0(lens, lens + n);
  rc = codec_decode(ctx, k, m, shards, lens, out, original_size, false);
  if (rc != RS_E_CORRUPT) return rc;
  // Verify failed: heal from the original presence, then join as rs_codec_decode does
  std::copy(lens0.begin(), lens0.end(), lens);
  int status = RS_OK;
  rc = heal_batch_host(ctx, k, m, max_errors, 1, shards, lens, healed, &status);
  if (rc) return rc;
  const size_t S = lens[0];
  if (static_cast<uint64_t>(S) * k < static_cast<uint64_t>(original_size)) return RS_E_INSUFFICIENT;
  size_t left = static_cast<size_t>(original_size);
  std::vector<CopyPool::Seg> segs;
  for (int i = 0; i < k && left; ++i) {
    const size_t c = std::min(S, left);
    segs.push_back({out + S * i, shards[i], c});
    left -= c;
  }
  ctx->pool.run(segs);
  return RS_OK;
}

int rs_codec_decode_heal(rs_ctx* ctx, int k, int m, uint8_t* const* shards, size_t* lens,
                         uint8_t* out, int64_t original_size, uint8_t* healed) {
  return rs_codec_decode_heal_ex(ctx, k, m, shards, lens, out, original_size, healed, 1);
}

// ---- exported: correct --------------------------------------------------

int rs_correct_batch(rs_ctx* ctx, int k, int m, int batch, uint8_t* const* shards, const size_t* lens,
                     uint64_t* counts, int* status) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || batch < 0 || (batch && (!shards || !lens || !counts || !status))) return RS_E_ARG;
  if ((rc = correct_batch_host(ctx, k, m, batch, shards, lens, counts, status))) return rc;
  return first_error(status, batch);
}

int rs_correct(rs_ctx* ctx, int k, int m, uint8_t* const* shards, const size_t* lens, uint64_t* counts) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || !shards || !lens || !counts) return RS_E_ARG;
  int status = RS_OK;
  if ((rc = correct_batch_host(ctx, k, m, 1, shards, lens, counts, &status))) return rc;
  return status;
}

int rs_codec_decode_correct(rs_ctx* ctx, int k, int m, uint8_t* const* shards, size_t* lens,
                            uint8_t* out, int64_t original_size, uint8_t* corrected) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || !shards || !lens || !corrected || original_size < 0 || (original_size && !out)) return RS_E_ARG;
  const size_t n = static_cast<size_t>(k + m);
  std::fill(corrected, corrected + n, 0);
  // the present shards are corrected where they can be; what the stripe's admission or a column
  // left over has to say is the decode's to say, with its own precedence
  std::vector<uint64_t> counts(n + 1, 0);
  int status = RS_OK;
  if ((rc = correct_batch_host(ctx, k, m, 1, shards, lens, counts.data(), &status))) return rc;
  for (size_t i = 0; i < n; ++i) corrected[i] = counts[i] != 0;
  return codec_decode(ctx, k, m, shards, lens, out, original_size, false);
}

// ---- exported: batched host-memory calls ------------------------------------------------

int rs_encode_batch(rs_ctx* ctx, int k, int m, int batch, const size_t* sizes,
                    const uint8_t* const* data, uint8_t* const* parity, int* status) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || batch < 0 || (batch && (!sizes || !data || !parity || !status))) return RS_E_ARG;
  const int n = k + m;
  const size_t B = static_cast<size_t>(batch);
  std::vector<uint8_t> present(B * n, 0);
  BatchGroups groups;
  for (size_t b = 0; b < B; ++b) {
    status[b] = sizes[b] ? RS_OK : RS_E_NO_DATA;  // upstream Encode: ErrShardNoData
    if (!sizes[b]) continue;
    std::memset(&present[b * n], 1, static_cast<size_t>(k));
    groups.add(sizes[b], &present[b * n], n, static_cast<int>(b));
  }
  std::vector<int> flags(B, 0);
  rc = run_batch(ctx, k, m, BatchMode{false, false}, groups, sizes, present.data(), nullptr,
                 [&](int b, int i) { return data[static_cast<size_t>(b) * k + i]; },
                 [&](int b, int i) { return parity[static_cast<size_t>(b) * m + i - k]; },
                 flags.data());
  if (rc) return rc;
  return first_error(status, batch);
}

int rs_reconstruct_batch(rs_ctx* ctx, int k, int m, int batch, uint8_t* const* shards,
                         size_t* lens, int verify, int* status) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || batch < 0 || (batch && (!shards || !lens || !status))) return RS_E_ARG;
  return reconstruct_batch_host(ctx, k, m, batch, shards, lens, verify != 0, nullptr, nullptr, status);
}

int rs_reconstruct_some_batch(rs_ctx* ctx, int k, int m, int batch, uint8_t* const* shards,
                              size_t* lens, const uint8_t* required, int verify, int* status) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || batch < 0 || (batch && (!shards || !lens || !status))) return RS_E_ARG;
  return reconstruct_batch_host(ctx, k, m, batch, shards, lens, verify != 0, nullptr, nullptr, status,
                                required);
}

// ---- exported: parity updated in place --------------------------------

int rs_update_batch(rs_ctx* ctx, int k, int m, int batch, const size_t* sizes,
                    const uint8_t* const* old_data, const uint8_t* const* new_data,
                    uint8_t* const* parity, int* status) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || batch < 0 || (batch && (!sizes || !new_data || !parity || !status))) return RS_E_ARG;
  if ((rc = update_batch_host(ctx, k, m, batch, sizes, old_data, new_data, parity, status))) return rc;
  return first_error(status, batch);
}

int rs_update(rs_ctx* ctx, int k, int m, size_t S, const uint8_t* const* old_data,
              const uint8_t* const* new_data, uint8_t* const* parity) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || !old_data || !new_data || !parity) return RS_E_ARG;
  // upstream Update: ErrInvalidInput for a new shard without its old one, before anything runs
  for (int i = 0; i < k; ++i)
    if (new_data[i] && !old_data[i]) return RS_E_ARG;
  int status = RS_OK;
  if ((rc = update_batch_host(ctx, k, m, 1, &S, old_data, new_data, parity, &status))) return rc;
  return status;
}

int rs_encode_idx(rs_ctx* ctx, int k, int m, size_t S, const uint8_t* shard, int idx,
                  uint8_t* const* parity) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || !shard || !parity || idx < 0 || idx >= k) return RS_E_ARG;  // upstream ErrInvalidShardIdx
  std::vector<const uint8_t*> one(static_cast<size_t>(k), nullptr);
  one[static_cast<size_t>(idx)] = shard;
  int status = RS_OK;
  if ((rc = update_batch_host(ctx, k, m, 1, &S, nullptr, one.data(), parity, &status))) return rc;
  return status;
}

// ---- exported: progressive decode --------------------------------------

// status[b]: the stripe's own refusal in the plan constructor's order -- the expect count
// (RS_E_TOO_FEW_SHARDS, RS_E_ARG), a misplaced pointer (RS_E_ARG), a zero size with both an input
// and a dst (RS_E_NO_DATA); the other stripes run. Stripes without an input or without a dst are
// RS_OK and reach no device.
int rs_decode_idx_batch(rs_ctx* ctx, int k, int m, int batch, const size_t* sizes, uint8_t* const* dst,
                        const uint8_t* expect, const uint8_t* const* input, unsigned flags, int* status) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || batch < 0 || (batch && (!sizes || !dst || !expect || !input || !status)) ||
      (flags & ~RS_DECODE_IDX_STORE))
    return RS_E_ARG;
  const size_t B = static_cast<size_t>(batch), n = static_cast<size_t>(k + m);
  std::vector<uint8_t> fl(B * n, 0);
  std::vector<int> ids;
  for (size_t b = 0; b < B; ++b) {
    int ne = 0;
    bool in = false, out = false, misplaced = false;
    for (size_t i = 0; i < n; ++i) {
      const size_t at = b * n + i;
      const bool e = expect[at] != 0;
      ne += e;
      in |= input[at] != nullptr;
      out |= dst[at] != nullptr;
      misplaced |= e ? dst[at] != nullptr : input[at] != nullptr;
      fl[at] = static_cast<uint8_t>((e ? 1 : 0) | (input[at] ? 2 : 0) | (dst[at] ? 4 : 0));
    }
    if (ne < k) status[b] = RS_E_TOO_FEW_SHARDS;
    else if (ne > k || misplaced) status[b] = RS_E_ARG;
    else if (!in || !out) status[b] = RS_OK;
    else if (sizes[b] == 0) status[b] = RS_E_NO_DATA;
    else {
      status[b] = RS_OK;
      ids.push_back(static_cast<int>(b));
    }
  }
  if ((rc = run_decode_idx<DecodeIdxTables>(ctx, k, m, (flags & RS_DECODE_IDX_STORE) != 0, false, ids, sizes,
                                            fl.data(),
                                            [&](int b, int i) { return input[static_cast<size_t>(b) * n + i]; },
                                            [&](int b, int i) { return dst[static_cast<size_t>(b) * n + i]; })))
    return rc;
  return first_error(status, batch);
}

int rs_decode_idx(rs_ctx* ctx, int k, int m, size_t S, uint8_t* const* dst, const uint8_t* expect,
                  const uint8_t* const* input, unsigned flags) {
  int status = RS_OK;
  const int rc = rs_decode_idx_batch(ctx, k, m, 1, &S, dst, expect, input, flags, &status);
  return rc ? rc : status;
}

// rs_decode_idx_batch with compared shards. A stripe in the launch -- an input
// and a wanted or check row, or under RS_DECODE_CHECK_FINAL a check row alone -- runs; a final
// call's flagged stripe is RS_E_CORRUPT, with its wanted rows delivered all the same.
int rs_decode_check_batch(rs_ctx* ctx, int k, int m, int batch, const size_t* sizes, uint8_t* const* dst,
                          uint8_t* const* check, const uint8_t* expect, const uint8_t* const* input,
                          unsigned flags, int* status) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || batch < 0 || (batch && (!sizes || !dst || !check || !expect || !input || !status)) ||
      (flags & ~(RS_DECODE_IDX_STORE | RS_DECODE_CHECK_FINAL)))
    return RS_E_ARG;
  const bool final = (flags & RS_DECODE_CHECK_FINAL) != 0;
  const size_t B = static_cast<size_t>(batch), n = static_cast<size_t>(k + m);
  std::vector<uint8_t> fl(B * n, 0);
  std::vector<int> ids;
  for (size_t b = 0; b < B; ++b) {
    int ne = 0;
    bool in = false, row = false, chk = false, misplaced = false;
    for (size_t i = 0; i < n; ++i) {
      const size_t at = b * n + i;
      const bool e = expect[at] != 0;
      ne += e;
      in |= input[at] != nullptr;
      row |= dst[at] != nullptr || check[at] != nullptr;
      chk |= check[at] != nullptr;
      misplaced |= e ? dst[at] != nullptr || check[at] != nullptr
                     : (input[at] != nullptr && !check[at]) || (check[at] != nullptr && dst[at] != nullptr);
      fl[at] = static_cast<uint8_t>((e ? 1 : 0) | (input[at] ? 2 : 0) | (dst[at] ? 4 : 0) | (check[at] ? 8 : 0));
    }
    if (ne < k) status[b] = RS_E_TOO_FEW_SHARDS;
    else if (ne > k || misplaced) status[b] = RS_E_ARG;
    else if (!((in && row) || (final && chk))) status[b] = RS_OK;
    else if (sizes[b] == 0) status[b] = RS_E_NO_DATA;
    else {
      status[b] = RS_OK;
      ids.push_back(static_cast<int>(b));
    }
  }
  std::vector<int> corrupt(B, 0);
  if ((rc = run_decode_idx<DecodeCheckTables>(
           ctx, k, m, (flags & RS_DECODE_IDX_STORE) != 0, final, ids, sizes, fl.data(),
           [&](int b, int i) { return input[static_cast<size_t>(b) * n + i]; },
           [&](int b, int i) {
             const size_t at = static_cast<size_t>(b) * n + i;
             return check[at] ? check[at] : dst[at];
           },
           corrupt.data())))
    return rc;
  for (int b : ids)
    if (corrupt[static_cast<size_t>(b)]) status[b] = RS_E_CORRUPT;
  return first_error(status, batch);
}

int rs_decode_check(rs_ctx* ctx, int k, int m, size_t S, uint8_t* const* dst, uint8_t* const* check,
                    const uint8_t* expect, const uint8_t* const* input, unsigned flags) {
  int status = RS_OK;
  const int rc = rs_decode_check_batch(ctx, k, m, 1, &S, dst, check, expect, input, flags, &status);
  return rc ? rc : status;
}

// The final rs_decode_check_batch call that repairs what it flags. status[b]:
// the stripe's own refusal in the plan constructor's order -- the expect count, a misplaced
// pointer (a fix at an index that is neither expected nor compared among them), more than 16
// rows (RS_E_UNSUPPORTED), a zero size in the launch -- while the other stripes run; RS_OK for a
// clean stripe and for one whose mismatching columns were all explained (counts say what was
// repaired); RS_E_CORRUPT when a column is unexplained, the wanted rows delivered all the same.
int rs_decode_repair_batch(rs_ctx* ctx, int k, int m, int batch, const size_t* sizes, uint8_t* const* dst,
                           uint8_t* const* check, uint8_t* const* fix, const uint8_t* expect,
                           const uint8_t* const* input, unsigned flags, int* status, uint64_t* counts) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || batch < 0 || (batch && (!sizes || !dst || !check || !fix || !expect || !input || !status)) ||
      (flags & ~RS_DECODE_IDX_STORE))
    return RS_E_ARG;
  const size_t B = static_cast<size_t>(batch), n = static_cast<size_t>(k + m);
  std::vector<uint8_t> fl(B * n, 0);
  std::vector<int> ids;
  for (size_t b = 0; b < B; ++b) {
    int ne = 0, rows = 0;
    bool in = false, chk = false, misplaced = false;
    for (size_t i = 0; i < n; ++i) {
      const size_t at = b * n + i;
      const bool e = expect[at] != 0;
      ne += e;
      in |= input[at] != nullptr;
      rows += dst[at] != nullptr || check[at] != nullptr;
      chk |= check[at] != nullptr;
      misplaced |= e ? dst[at] != nullptr || check[at] != nullptr
                     : (input[at] != nullptr && !check[at]) || (check[at] != nullptr && dst[at] != nullptr) ||
                           (fix[at] != nullptr && !check[at]);
      fl[at] = static_cast<uint8_t>((e ? 1 : 0) | (input[at] ? 2 : 0) | (dst[at] ? 4 : 0) | (check[at] ? 8 : 0) |
                                    (fix[at] ? 16 : 0));
    }
    if (ne < k) status[b] = RS_E_TOO_FEW_SHARDS;
    else if (ne > k || misplaced) status[b] = RS_E_ARG;
    else if (rows > kRepairRows) status[b] = RS_E_UNSUPPORTED;
    else if (!((in && rows) || chk)) status[b] = RS_OK;
    else if (sizes[b] == 0) status[b] = RS_E_NO_DATA;
    else {
      status[b] = RS_OK;
      ids.push_back(static_cast<int>(b));
    }
  }
  std::vector<uint64_t> own;
  if (!counts) {
    own.assign(B * (n + 1), 0);
    counts = own.data();
  } else {
    std::fill(counts, counts + B * (n + 1), 0);
  }
  std::vector<int> corrupt(B, 0);
  if ((rc = run_decode_repair(
           ctx, k, m, (flags & RS_DECODE_IDX_STORE) != 0, ids, sizes, fl.data(),
           [&](int b, int i) { return input[static_cast<size_t>(b) * n + i]; },
           [&](int b, int i) {
             const size_t at = static_cast<size_t>(b) * n + i;
             return check[at] ? check[at] : dst[at];
           },
           [&](int b, int i) { return fix[static_cast<size_t>(b) * n + i]; }, counts, corrupt.data())))
    return rc;
  for (int b : ids)
    if (counts[static_cast<size_t>(b) * (n + 1) + n]) status[b] = RS_E_CORRUPT;
  return first_error(status, batch);
}

int rs_decode_repair(rs_ctx* ctx, int k, int m, size_t S, uint8_t* const* dst, uint8_t* const* check,
                     uint8_t* const* fix, const uint8_t* expect, const uint8_t* const* input, unsigned flags,
                     uint64_t* counts) {
  int status = RS_OK;
  const int rc = rs_decode_repair_batch(ctx, k, m, 1, &S, dst, check, fix, expect, input, flags, &status, counts);
  return rc ? rc : status;
}

int rs_codec_overwrite(rs_ctx* ctx, int k, int m, size_t S, uint8_t* const* shards, int64_t offset,
                       const uint8_t* data, size_t len) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || !shards || !data || offset < 0) return RS_E_ARG;
  std::vector<OverwriteInterval> iv;
  if (!overwrite_plan(k, S, static_cast<uint64_t>(offset), len, iv)) return RS_E_ARG;
  const size_t K = static_cast<size_t>(k), M = static_cast<size_t>(m);
  const size_t first = static_cast<size_t>(offset) / S, last = (static_cast<size_t>(offset) + len - 1) / S;
  for (size_t i = first; i <= last; ++i)
    if (!shards[i]) return RS_E_ARG;
  for (size_t j = 0; j < M; ++j)
    if (!shards[K + j]) return RS_E_ARG;
  // one stripe per column interval: its changed shards' old bytes in the shards, their new
  // bytes in `data`, its parity columns
  const size_t B = iv.size();
  std::vector<size_t> sizes(B);
  std::vector<const uint8_t*> old_data(B * K, nullptr), new_data(B * K, nullptr);
  std::vector<uint8_t*> parity(B * M);
  for (size_t b = 0; b < B; ++b) {
    sizes[b] = iv[b].col1 - iv[b].col0;
    for (int i = iv[b].shard0; i <= iv[b].shard1; ++i) {
      old_data[b * K + i] = shards[i] + iv[b].col0;
      new_data[b * K + i] = data + (static_cast<size_t>(i) * S + iv[b].col0 - static_cast<size_t>(offset));
    }
    for (size_t j = 0; j < M; ++j) parity[b * M + j] = shards[K + j] + iv[b].col0;
  }
  std::vector<int> status(B, RS_OK);
  if ((rc = update_batch_host(ctx, k, m, static_cast<int>(B), sizes.data(), old_data.data(),
                              new_data.data(), parity.data(), status.data())))
    return rc;
  if ((rc = first_error(status.data(), static_cast<int>(B)))) return rc;
  // the parity is new: now the data shards
  std::vector<CopyPool::Seg> segs;
  for (size_t i = first; i <= last; ++i) {
    const size_t lo = std::max(static_cast<size_t>(offset), i * S);
    const size_t hi = std::min(static_cast<size_t>(offset) + len, (i + 1) * S);
    segs.push_back({shards[i] + (lo - i * S), data + (lo - static_cast<size_t>(offset)), hi - lo});
  }
  ctx->pool.run(segs);
  return RS_OK;
}

// ---- exported: codec-level batches (objects in, objects out) ----------------------------

// rs_codec_encode_batch, and with digests (batch * n * 32 bytes) rs_codec_encode_batch_sums.
static int codec_encode_batch(rs_ctx* ctx, int k, int m, int batch, const uint8_t* const* data,
                              const size_t* lens, uint8_t* const* shards_out, const size_t* out_caps,
                              size_t* shard_sizes, int* status, uint8_t* digests, bool with_sums) {
  DeviceGuard dg;
  // per object codec.go:31 Split and :36 Encode; the profile (:22-26) is the call's
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || batch < 0 ||
      (batch && (!data || !lens || !shards_out || !out_caps || !shard_sizes || !status ||
                 (with_sums && !digests))))
    return RS_E_ARG;
  const int n = k + m;
  const size_t B = static_cast<size_t>(batch);
  std::vector<uint8_t> present(B * n, 0);
  std::vector<SplitPlan> plan(B);
  std::vector<size_t> S(B, 0);  // nonzero for the stripes that run
  std::vector<Join> tees(B, Join{nullptr, 0, 0, k});
  BatchGroups groups;
  for (size_t b = 0; b < B; ++b) {
    if (lens[b] == 0) {
      status[b] = RS_E_SHORT_DATA;  // upstream Split
      continue;
    }
    plan[b] = split_plan(k, lens[b]);
    if (!data[b] || !shards_out[b] || out_caps[b] / static_cast<size_t>(n) < plan[b].S) {
      status[b] = RS_E_ARG;
      continue;
    }
    status[b] = RS_OK;
    shard_sizes[b] = S[b] = plan[b].S;
    split_prepare(plan[b], n, data[b], shards_out[b]);
    tees[b] = split_tee(plan[b], shards_out[b]);
    for (int i = 0; i < k; ++i) present[b * n + i] = 1;
    groups.add(S[b], &present[b * n], n, static_cast<int>(b));
  }
  std::vector<int> flags(B, 0);
  SumsCall sums;
  sums.mode = SumsMode::kDigest;
  sums.n = n;
  sums.digests = digests;
  rc = run_batch(ctx, k, m, BatchMode{false, false}, groups, S.data(), present.data(), tees.data(),
                 [&](int b, int i) { return split_row(plan[b], data[b], shards_out[b], i); },
                 [&](int b, int i) { return shards_out[b] + S[b] * static_cast<size_t>(i); },
                 flags.data(), with_sums ? &sums : nullptr);
  if (rc) return rc;
  return first_error(status, batch);
}

int rs_codec_encode_batch(rs_ctx* ctx, int k, int m, int batch, const uint8_t* const* data,
                          const size_t* lens, uint8_t* const* shards_out, const size_t* out_caps,
                          size_t* shard_sizes, int* status) {
  return codec_encode_batch(ctx, k, m, batch, data, lens, shards_out, out_caps, shard_sizes, status,
                            nullptr, false);
}

int rs_codec_encode_batch_sums(rs_ctx* ctx, int k, int m, int batch, const uint8_t* const* data,
                               const size_t* lens, uint8_t* const* shards_out, const size_t* out_caps,
                               size_t* shard_sizes, uint8_t* digests, int* status) {
  return codec_encode_batch(ctx, k, m, batch, data, lens, shards_out, out_caps, shard_sizes, status,
                            digests, true);
}

int rs_codec_decode_batch(rs_ctx* ctx, int k, int m, int batch, uint8_t* const* shards,
                          size_t* lens, uint8_t* const* out, const int64_t* original_sizes,
                          int* status) {
  DeviceGuard dg;
  // per object codec.go:55 Reconstruct, :59-65 Verify, :67-77 join / trim
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || batch < 0 || (batch && (!shards || !lens || !out || !original_sizes || !status)))
    return RS_E_ARG;
  return reconstruct_batch_host(ctx, k, m, batch, shards, lens, true, out, original_sizes, status);
}

int rs_codec_decode_batch_sums(rs_ctx* ctx, int k, int m, int batch, uint8_t* const* shards,
                               size_t* lens, const uint8_t* expected, uint8_t* const* out,
                               const int64_t* original_sizes, uint8_t* bad, int* status) {
  DeviceGuard dg;
  // per object manager.go:283-296 (a shard whose checksum differs counts as missing), then
  // codec.go:55 Reconstruct, :59-65 Verify, :67-77 join / trim
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || batch < 0 ||
      (batch && (!shards || !lens || !expected || !out || !original_sizes || !bad || !status)))
    return RS_E_ARG;
  return reconstruct_batch_host(ctx, k, m, batch, shards, lens, true, out, original_sizes, status,
                                nullptr, false, expected, bad);
}

int rs_codec_decode_data_batch(rs_ctx* ctx, int k, int m, int batch, uint8_t* const* shards,
                               size_t* lens, uint8_t* const* out, const int64_t* original_sizes,
                               int* status) {
  DeviceGuard dg;
  int rc = check_profile(k, m);
  if (rc) return rc;
  if (!ctx || batch < 0 || (batch && (!shards || !lens || !out || !original_sizes || !status)))
    return RS_E_ARG;
  return reconstruct_batch_host(ctx, k, m, batch, shards, lens, true, out, original_sizes, status,
                                nullptr, true);
}

}  // extern "C"
