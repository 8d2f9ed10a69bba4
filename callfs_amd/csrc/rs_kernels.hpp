// Launch interface of the GF(2^8) shard-matrix kernels (rs_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <vector>
#include <cstdint>

#include "absorb_tables.hpp"
#include "order_code.hpp"

// 1: also build the measurement-only kernel forms (the 6-bit triple lookups, the 64-vector
// and double-buffered realigning forms, the no-lookup and aligned-window ceilings) and honour
// the A/B environment toggles (CALLFS_RS_WIX, _TRIDB, _REALIGN, _TAIL_LAST_TPS). The
// product library is built with 0: `python callfs_amd/build.py --ab` writes the A/B build to
// libcallfs_rs_ab.so, which the development tools load through CALLFS_RS_LIB.
#ifndef CALLFS_RS_AB_INSTANCES
#define CALLFS_RS_AB_INSTANCES 0
#endif

namespace callfs {

constexpr bool kAbInstances = CALLFS_RS_AB_INSTANCES != 0;

constexpr int kMaxRowsPerLaunch = 16;  // output rows per launch group (LDS kernel above 4)
constexpr int kMaxK = 256;

// One launch applies an R x K coefficient block to every stripe of a batch:
//   out[b][r][x] = XOR_i coef[r][i] * in[b][i][x]      for x in [0, S)
// Rows with bit r of verify_mask set are compared against out[b][r] instead of
// stored; any mismatch ORs 1 into *status (upstream Verify, codec.go:59).
struct ApplyArgs {
  const uint8_t* const* in_tab;  // [batch][K] device pointers (k valid shards)
  uint8_t* const* out_tab;       // [batch][R] device pointers (written or compared)
  const uint32_t* tabs;          // [K][R][5] v_perm tables (gf256.hpp perm_tables)
  const uint8_t* ltabs;          // [K][32][W] nibble tables for rs_apply_lds (gf256.hpp nibble_tables)
  uint64_t S;                    // shard bytes
  uint64_t nvec;                 // 16-byte vectors per shard handled by the vector kernel
  uint32_t verify_mask;
  int* status;                   // mismatch flag; stripe b uses status[b * status_stride]
  int status_stride;
  int K;
  int R;
  int batch;
  // log2 of the largest power of two dividing every difference between the shard
  // addresses of a stripe (shard_addr_tz); picks the LDS kernel's tile order. 0 = odd
  // or unknown.
  int addr_tz;
  // byte distance between consecutive stripes' shards when it is the same for every
  // stripe (0 = one stripe or irregular); also keys the tile order.
  uint64_t stripe_stride;
  // first tile of this launch (launch_apply cuts grids of many tiles into consecutive
  // slices; a kernel's block b works on tile t_base + b of the whole tile order)
  uint32_t t_base;
  // OR of (address & 15) over every input shard pointer of every stripe: nonzero when
  // some input shard is not 16-B aligned (upstream Split layout of a contiguous object
  // at odd S); selects the LDS kernel's realigning form (rs_apply.hpp REALIGN)
  uint32_t in_misalign;
  // the same over the launch group's output (written or compared) shard pointers; with
  // in_misalign it selects the form that also aligns the parity stores (REALIGN 2)
  uint32_t out_misalign;
  // set by launch_apply: nonzero when the vector kernel also computes the ragged tail S % 16
  // (no separate byte-kernel launch): (tile << 2) | (last wave << 1) | 1, the tile of each
  // stripe and the wave (0 or the block's last) that take it (rs_apply.hpp tail_lane)
  uint32_t tail_in_vec;
  // host-side handle of the launch group's bit-sliced kernel (bitslice.hpp bs::Kernel, compiled
  // at plan time for this coefficient block) or null; the device kernels never read it
  const void* bs;
};

// One-dispatch small host calls (rs_apply_small): stripe b's shard i lives at
// base + b*spitch + i*cpitch in host-coherent pinned staging that the kernel reads and
// writes over PCIe; one launch group (R <= 16 rows) per launch.
struct SmallArgs {
  const uint8_t* base;
  uint64_t spitch;       // bytes per stripe in staging
  uint64_t cpitch;       // bytes per shard (S rounded up to 16)
  uint32_t nvec;         // 16-B vectors per shard, ceil(S / 16)
  uint32_t S;
  int K;
  int R;
  int batch;
  uint32_t verify_mask;
  // device memory, uploaded once per (lane, tables): [K][R][5] v_perm tables of the group,
  // then idx: the shard index of input i (idx[i], the k valid shards) and of row r
  // (idx[256 + r]). Kept out of the kernel arguments: 272 B of arguments cost the launch
  // ~2 us (profiles/r03/small_path/r03_smalltrace2)
  const uint32_t* tabs;
  const uint8_t* idx;
  // idx[0..15] and idx[256..271] again, as kernel arguments: the data loads of a k <= 16
  // call need no dependent device-memory read first
  uint32_t idx_in[4];
  uint32_t idx_out[4];
  int* status;           // host-coherent: status[b] = 1 when stripe b's Verify rows mismatch
  // completion flag (last launch of a call only, else null): when every block of the launch
  // has finished, the last one stores `seq` into *done (host-coherent) with a system-scope
  // release; `counter` (device memory, 0 between launches) counts finished blocks
  int* done;
  unsigned* counter;
  int seq;
};

// Enqueues rs_apply_small for one launch group on `stream`.
hipError_t launch_small(const SmallArgs& a, hipStream_t stream);

// One-dispatch small ragged batches (rs_apply_small_ragged): a chunk of items of different
// widths and patterns in host-coherent staging (ragged_chunks.hpp), one launch group per
// launch. Item j's table entry is four dwords in the staging buffer itself: {offset of its
// input rows / 16, offset of its output rows / 16, width in bytes, pattern}; rows are pitched
// at the width rounded up to 16. Input row i is the pattern's i-th read shard (the k valid
// ones, then the compared ones); row rho of the pattern is output row rho when written and
// input row K + rho - missing when compared.
struct SmallRaggedArgs {
  const uint8_t* base;    // the chunk's staging
  const uint32_t* items;  // [nitems][4], inside the staging buffer
  // device memory, cached per lane: pattern p's block of this launch group at
  // ptabs + p * pstride dwords: {compare mask, missing count, 0, 0}, then [K][R][5] v_perm tables
  const uint32_t* ptabs;
  uint32_t pstride;
  uint32_t max_nvec;  // 16-B vectors of the widest item
  int K;
  int R;
  int row0;  // first pattern row of this launch group
  int nitems;
  int* status;  // host-coherent: status[j] = 1 when item j's compared rows mismatch
  // completion flag and counter as in SmallArgs
  int* done;
  unsigned* counter;
  int seq;
};

// Enqueues rs_apply_small_ragged for one launch group on `stream`.
hipError_t launch_small_ragged(const SmallRaggedArgs& a, hipStream_t stream);

// addr_tz for a set of shard addresses: trailing zeros of the OR of their differences
// from the first (63 for a single address).
inline int shard_addr_tz(const void* const* p, int count) {
  uint64_t d = 0;
  for (int i = 1; i < count; ++i)
    d |= reinterpret_cast<uintptr_t>(p[i]) ^ reinterpret_cast<uintptr_t>(p[0]);
  return d ? __builtin_ctzll(d) : 63;
}

// [0, 16*floor(S/16)) runs on a vector kernel and the ragged tail on the byte kernel,
// whatever the pointers' alignment: gfx950 under ROCm (SH_MEM_CONFIG alignment mode
// "unaligned") serves 16-byte global accesses at any byte address, and at odd shard
// offsets (upstream Split layout of a contiguous object) that ran 4.7x the byte kernel
// (DESIGN.md §5). bytes_only forces the byte kernel over all of [0, S) (kbench A/B).
// Returns hipSuccess or the launch error.
// `order` arguments below are order codes (order_code.hpp: the kOrder* bands and their decoder).
constexpr int kBitsliceMinRows = 1;

// `order` >= 0 (a TileOrder) replaces the measured rule for this launch where the
// chosen kernel has an instance in that order (order_candidates lists them); -1 = the
// rule (or CALLFS_RS_TILE_ORDER).
// ev_start / ev_stop (optional, created by the caller): recorded by the launch's first
// kernel dispatch when it starts and by its last when it ends (hipExtLaunchKernel), so
// their interval is the kernels' own time without the stream's gaps before and after.
struct LaunchEvents {
  hipEvent_t start = nullptr;
  hipEvent_t stop = nullptr;
};
hipError_t launch_apply(ApplyArgs a, hipStream_t stream, bool bytes_only = false, int order = -1,
                        LaunchEvents ev = {});

// Tile orders worth timing for launch `a` (rs_plan_tune): the rule's choice first, then
// the alternatives that have kernel instances for this path. Empty when the launch has
// no choice (byte kernel, realigning kernel, S < 16). every_instance: also the orders
// that have an instance but never measured faster (rs_plan_set_orders accepts them).
std::vector<int> order_candidates(const ApplyArgs& a, bool every_instance = false);

// True when the rule runs launch `a` on its bit-sliced kernel (ApplyArgs::bs) once that is
// compiled (rs_plan_create compiles it up front for such launches).
bool bitslice_wanted(const ApplyArgs& a);

// The form (an order code as order_candidates lists them) launch_apply runs for `order`
// (-1 = the tune table's entry for the launch's shape, else the rule, whose bit-sliced choice
// counts once its kernel is compiled).
int launch_form(const ApplyArgs& a, int order);

// The tune table (tune_table.hpp): the order rs_plan_tune measured for launch `a`'s shape on
// the current device, when it is one `a` offers and (for a bit-sliced order) its kernel is
// compiled -- else -1, and the rule decides. record_tuned stores a tuner's choice.
int tuned_order(const ApplyArgs& a);
void record_tuned(const ApplyArgs& a, int order);

// Measurement only (rs_plan_launch_ceiling), for launch `a` in the order the production
// launch takes (`order` as for launch_apply), on the production grid and slicing:
//   mode 0  the no-lookup form of the LDS kernel: same loads, stores and table prologue,
//           one XOR per input dword instead of the lookups (outputs junk, Verify rows may
//           flag status);
//   mode 1  the launch's read streams alone (inputs + Verify rows; writes nothing);
//   mode 2  its write streams alone (junk into the written rows);
//   modes 3..8 (probes) the write / read streams from each row's first 64 / 128 / 256-B
//           boundary.
// Modes 0 and 3..8 exist in the A/B build only (hipErrorNotSupported otherwise).
hipError_t launch_ceiling(ApplyArgs a, hipStream_t stream, int order, int mode,
                          LaunchEvents ev = {});


// ---- mixed launches (rs_mixed.hip) --------------------------------------
// One launch group of a batch whose stripes have different erasure patterns: stripe b runs
// pattern p = pat[b], whose nibble tables sit at a.ltabs + p * tab_stride and whose compare
// mask is vmask[p] (a.verify_mask is not read; a.tabs and a.bs are unused). Host side:
// mixed_tables.hpp.
struct MixedArgs {
  const uint32_t* pat;    // [batch] pattern of each stripe
  const uint32_t* vmask;  // [P] verify mask of each pattern for this launch group
  uint32_t tab_stride;    // bytes between two patterns' tables (a multiple of 256)
};

// (kOrderMixed + the TileOrder it runs in, always consecutive: rs_plan_forms of a mixed plan)
constexpr int kOrderMixed = 512;

// Enqueues the launch group: the mixed nibble-table kernel over [0, S) for S >= 16 (the
// S % 16 tail inside it, unaligned 16-B accesses on misaligned shards), the mixed byte
// kernel for S < 16. Consecutive tile order, sliced like launch_apply; never the bit-sliced
// path, the tune table or a tile-order rule. ev as for launch_apply.
hipError_t launch_mixed(ApplyArgs a, const MixedArgs& x, hipStream_t stream, LaunchEvents ev = {});

// ---- ragged launches (rs_mixed.hip) -------------------------------------
// One launch group of a batch whose stripes have different shard sizes as well as different
// erasure patterns. Tile t of the launch belongs to stripe s = tile_stripe[t] and is tile
// t - tile0[s] of it; the stripe's shard size is size[s] and its pattern pat[s], with tables
// and compare mask as in MixedArgs (a.S, a.nvec and a.verify_mask are not read). Host side:
// ragged_tables.hpp.
struct RaggedArgs {
  const uint32_t* pat;          // [batch] pattern of each stripe
  const uint32_t* vmask;        // [P] verify mask of each pattern for this launch group
  const uint64_t* size;         // [batch] shard bytes of each stripe (>= 1)
  const uint32_t* tile0;        // [batch + 1] first tile of each stripe
  const uint32_t* tile_stripe;  // [ntiles] owning stripe of each tile
  uint32_t tab_stride;          // bytes between two patterns' tables (a multiple of 256)
  uint32_t ntiles;              // tile0[batch]
};

// (kOrderRagged + the TileOrder it runs in, always consecutive: rs_plan_forms of a ragged plan)
constexpr int kOrderRagged = 1024;
// 16-byte vectors per tile of the tile map (the mixed instances' tile)
constexpr uint32_t kRaggedLaunchTileVecs = 512;

// Enqueues the launch group: the ragged nibble-table kernel over every stripe's [0, size),
// each stripe's size % 16 tail inside it when any_tail (a stripe shorter than 16 bytes is one
// tile that is all tail), unaligned 16-B accesses on misaligned shards. Consecutive tile
// order, sliced like launch_mixed; never the bit-sliced path, the tune table or a tile-order
// rule. ev as for launch_apply. nrows (nullable): the patterns' row counts of a required launch
// (RaggedSomeArgs below), which runs the required kernel; x.ntiles == 0 then enqueues nothing.
hipError_t launch_ragged(ApplyArgs a, const RaggedArgs& x, const uint32_t* nrows, bool any_tail,
                         hipStream_t stream, LaunchEvents ev = {});

// ---- required launches (rs_mixed.hip) ----------------------------------
// A ragged launch group whose patterns have their own row counts (ReconstructSome: a
// missing shard nobody wants has no row). r is the launch group's own tile map, over the
// stripes with a row in the group alone (tile0 still indexed by stripe); nrows[p] in 1..a.R
// is how many of pattern p's rows the group holds. out_tab is pitched at a.R, and slots at
// and past a stripe's row count hold nothing the kernel loads.
struct RaggedSomeArgs {
  RaggedArgs r;
  const uint32_t* nrows;  // [P] rows of each pattern in this launch group
};

// (kOrderRequired + the TileOrder it runs in, always consecutive: rs_plan_forms of a required plan)
constexpr int kOrderRequired = 2048;

// ---- update launches (rs_update.hpp in rs_mixed.hip) ---------------------
// Upstream Update / EncodeIdx: a ragged launch group whose rows start from the destination's
// current bytes. Stripe s reads the nsrc[pat[s]] changed shards of its pattern alone and does
//   out[s][r] ^= XOR_{i < nsrc} coef[r][i] * d_i,   d_i = old_i ^ new_i (pair) or the shard (single)
// in_tab is pitched at in_stride pointers per stripe: source i of a pair launch is
// (in_tab[s][2i], in_tab[s][2i + 1]) = (old, new), of a single launch in_tab[s][i]. The tile
// map holds only the stripes with a changed shard; a.K is the largest source count of a
// pattern (the tables' pitch and the LDS size), out_tab is pitched at a.R. No verify mask and
// no status word: a.status, vmask and a.verify_mask are not read.
struct UpdateArgs {
  const uint32_t* pat;          // [batch] pattern of each stripe
  const uint32_t* nsrc;         // [P] changed shards of each pattern, 1..a.K
  const uint64_t* size;         // [batch] shard bytes of each stripe (>= 1 where it has a tile)
  const uint32_t* tile0;        // [batch + 1] first tile of each stripe
  const uint32_t* tile_stripe;  // [ntiles] owning stripe of each tile
  uint32_t tab_stride;          // bytes between two patterns' tables (a multiple of 256)
  uint32_t ntiles;
  uint32_t in_stride;           // pointers per stripe in in_tab: a.K, or 2 * a.K for pairs
};

// (kOrderUpdate + the TileOrder it runs in, always consecutive: rs_plan_forms of an update plan)
constexpr int kOrderUpdate = 4096;

// Enqueues the launch group: rs_update_ragged over every mapped stripe's [0, size), the
// size % 16 tails inside it when any_tail, unaligned 16-B accesses on misaligned shards.
// Consecutive tile order, sliced like launch_ragged; x.ntiles == 0 enqueues nothing. NOT
// idempotent: every launch applies the delta again. ev as for launch_apply.
hipError_t launch_update(ApplyArgs a, const UpdateArgs& x, bool pair, bool any_tail,
                         hipStream_t stream, LaunchEvents ev = {});

// ---- decode-idx launches (rs_merge.hpp in rs_mixed.hip) ------------------
// Upstream DecodeIdx: a single-source update launch group whose patterns have their own row
// counts and whose rows are either merged into the destination or stored over it. Stripe s
// reads the nsrc[pat[s]] delivered shards of its pattern and does, for r < nrows[pat[s]],
//   out[s][r] ^= XOR_{i < nsrc} coef[r][i] * in[s][i]   (merge)
//   out[s][r]  = XOR_{i < nsrc} coef[r][i] * in[s][i]   (store: the destination is never read)
// u as for a single launch_update (in_stride = a.K); out_tab is pitched at a.R, the most rows a
// pattern has in this launch group, and slots at and past a stripe's row count hold nothing the
// kernel loads. A mapped stripe whose pattern has nrows 0 in this group is left untouched.
struct MergeArgs {
  UpdateArgs u;
  const uint32_t* nrows;  // [P] rows of each pattern in this launch group, 0..a.R
};

// (kOrderDecodeIdx + the TileOrder it runs in, always consecutive: rs_plan_forms of a decode-idx plan)
constexpr int kOrderDecodeIdx = 32768;

// Enqueues the launch group: rs_merge_ragged (store: its STORE instances) over every mapped
// stripe's [0, size), tails, misaligned shards, order and slicing as launch_update;
// x.u.ntiles == 0 enqueues nothing. A merge launch is NOT idempotent; a store launch is.
hipError_t launch_decode_idx(ApplyArgs a, const MergeArgs& x, bool store, bool any_tail,
                             hipStream_t stream, LaunchEvents ev = {});

// ---- final decode-check launches (rs_check.hpp in rs_mixed.hip) ----------
// Progressive Verify: a decode-idx launch group in which some rows are check rows, syndrome
// accumulators that the final launch tests instead of writing. For r < nrows[pat[s]] with bit r
// of cmask[pat[s]] set, the value out[s][r] would have received (merge: its bytes XOR the
// computed row; store: the computed row, out[s][r] never read) is tested byte by byte, nothing is
// stored, and a nonzero byte ORs 1 into status[s * status_stride]; the other rows are merged or
// stored as by launch_decode_idx. A pattern may have no source at all (nsrc 0, and a.K 0 when no
// pattern has one): its rows' current bytes are what is tested (merge) and nothing else moves.
struct CheckArgs {
  MergeArgs m;
  const uint32_t* cmask;  // [P] bit r: row r of pattern p in this launch group is a check row
};

// Enqueues the launch group: rs_check_ragged (store: its STORE instances) over every mapped
// stripe's [0, size); a.status is required; tails, misaligned shards, order and slicing as
// launch_decode_idx (rs_plan_forms: kOrderDecodeCheck of order_code.hpp + consecutive);
// x.m.u.ntiles == 0 enqueues nothing. A merge launch with a row that is no check row is NOT
// idempotent; every other launch is.
hipError_t launch_decode_check(ApplyArgs a, const CheckArgs& x, bool store, bool any_tail,
                               hipStream_t stream, LaunchEvents ev = {});

// ---- decode-repair launches (rs_repair.hpp in rs_mixed.hip) --------------
// A final decode-check launch group that repairs what its check rows explain. Every pattern's
// check rows are its rows [0, nchk[p]) (c.cmask[p] is the low nchk[p] bits) and every stripe has
// at most 16 rows. A byte column's check values are its syndromes: locate_correct
// (locate_tables.hpp) over them names an expected shard at position j with error e -- every
// wanted row r, stored as computed, then gets G[r][j] . e XORed in where it lies, by the lane
// that stored it -- or a compared shard x with
// error s_x, or leaves the column unexplained (always, with fewer than 3 check rows). The error
// value is XORed into the byte of fix[s * (k + 16) + position] when that pointer is non-null,
// columns are added per verdict into counts[s * nbins + shard] (unexplained: bin nbins - 1) and
// a stripe with a mismatching column has 1 ORed into its status word, repaired or not. Check
// rows are never written.
struct RepairArgs {
  CheckArgs c;
  const uint8_t* gf;    // log[256], exp[512]
  const uint8_t* loc;   // [P] pattern blocks of loc_stride bytes (decode_repair_tables.hpp)
  uint64_t* counts;     // [batch][nbins]
  uint8_t* const* fix;  // [batch][k + 16] by position: expected V[j], then compared x; null allowed
  uint32_t loc_stride;  // locate_stride(k)
  uint32_t nbins;       // k + m + 1
  int k;                // the code's k: positions below it are expected shards
};

// (kOrderDecodeRepair of order_code.hpp + consecutive: rs_plan_forms of a decode-repair plan.)
// Enqueues the launch group: rs_repair_ragged (store: its STORE instances) over every mapped
// stripe's [0, size); arguments, tails, misaligned shards, order and slicing as
// launch_decode_check. Counts accumulate from launch to launch. A merge launch with a wanted row
// is NOT idempotent, nor is a launch with a fix row; every other launch is.
hipError_t launch_decode_repair(ApplyArgs a, const RepairArgs& x, bool store, bool any_tail,
                                hipStream_t stream, LaunchEvents ev = {});

// ---- feed launches (rs_feed.hpp in rs_mixed.hip) -------------------------
// One delivered shard of one stripe into the stripe's R <= 16 resident rows:
//   row[r] ^= c[r] * src   (merge; a row with c[r] == 0 is neither read nor written)
//   row[r]  = c[r] * src   (store: no row byte is read)
// over [0, S), with c the column of the shard's table block. The kernel's second argument: the
// source and, for instances of up to 8 rows, the row pointers by value (the 16-row instance reads
// them from FeedArgs::row_tab).
template <int RT>
struct FeedRows {
  const uint8_t* src;
  uint8_t* row[RT > 8 ? 1 : RT];
};

struct FeedArgs {
  const uint8_t* src;       // S bytes the device can read, any alignment
  const uint32_t* tabs;     // device memory: the shard's block, [R][5] v_perm tables
  uint8_t* const* row_tab;  // device memory: the R row pointers
  uint8_t* const* rows;     // host memory: the same R pointers
  uint64_t S;
  int R;
};

// bytes of the source, and of every row, that one block of a feed launch covers
constexpr uint32_t kFeedTileBytes = 4096;

// Enqueues rs_feed (store: its STORE instances) in the smallest instance that holds R rows, on a
// grid of ceil(S / kFeedTileBytes) blocks: one dispatch, no allocation, no copy, no sync. R == 0
// enqueues nothing. A merge launch is NOT idempotent; a store launch is.
hipError_t launch_feed(const FeedArgs& x, bool store, hipStream_t stream, LaunchEvents ev = {});

// ---- absorb launches (rs_absorb.hpp in rs_mixed.hip) ----------------------
// One range [off, off + len) of an object's body into the object's R <= 16 resident parity rows:
//   row[j][c] ^= P[j][i] * src[i * S + c - off]   for every byte (shard i, column c) of the range
// and nothing else. The kernel's second argument: the source, the range's first byte, the plan's
// intervals and block counts and, for instances of up to 8 rows, the row pointers, all by value
// (the 16-row instance reads the pointers from AbsorbArgs::row_tab).
template <int RT>
struct AbsorbRows {
  const uint8_t* src;
  uint64_t off;
  AbsorbInterval iv[kAbsorbMaxIntervals];
  uint32_t end[kAbsorbMaxIntervals];
  uint8_t* row[RT > 8 ? 1 : RT];
};

struct AbsorbArgs {
  const uint8_t* src;       // len bytes the device can read, any alignment: body byte off + b at src[b]
  const uint32_t* tabs;     // device memory: the arena, [K][R][5] v_perm tables
  uint8_t* const* row_tab;  // device memory: the R row pointers
  uint8_t* const* rows;     // host memory: the same R pointers
  uint64_t S, off, len;
  int K, R;
  AbsorbPlan plan;          // absorb_plan(K, S, off, len)
};

// Enqueues rs_absorb in the smallest instance that holds R rows, on a grid of the plan's blocks
// (the sum of the intervals' ceil(columns / kFeedTileBytes)): one dispatch, no allocation, no
// copy, no sync. The plan is checked against K, S, off and len before anything is enqueued. NOT
// idempotent.
hipError_t launch_absorb(const AbsorbArgs& x, hipStream_t stream, LaunchEvents ev = {});

// ---- locate launches (rs_mixed.hip) --------------------------------------
// A required launch group in which every row is compared and none written, and a mismatching
// byte column is classified instead of only flagged: locate_classify (locate_tables.hpp) turns
// its a.R' syndromes into the shard to blame or "unexplained", and the kernel adds the columns
// per verdict into counts[stripe * nbins + shard] (unexplained: bin nbins - 1). r, nrows and
// out_tab as in RaggedSomeArgs; the status words are ORed as in every compare. Sums are formed
// per wave and only nonzero ones reach memory, as 64-bit atomic adds; no shard byte is written.
struct LocateArgs {
  RaggedArgs r;
  const uint32_t* nrows;  // [P] compared rows r' of each pattern, 1..a.R for a mapped stripe
  const uint8_t* gf;      // log[256], exp[512]
  const uint8_t* loc;     // [P] pattern blocks of loc_stride bytes (locate_tables.hpp kLoc*)
  uint64_t* counts;       // [batch][nbins]
  uint32_t loc_stride;
  uint32_t nbins;         // k + m + 1
};

// (kOrderLocate + the TileOrder it runs in, always consecutive: rs_plan_forms of a locate plan)
constexpr int kOrderLocate = 8192;

// Enqueues the launch group: rs_apply_locate over every mapped stripe's [0, size), tails and
// misaligned shards as launch_ragged. Consecutive tile order, sliced like launch_ragged;
// x.r.ntiles == 0 enqueues nothing. Counts accumulate from launch to launch. ev as for
// launch_apply. max_errors 2 (a pair plan, §5.12.1): rs_apply_locate2, with x.gf the
// kLoc2GfBytes block, x.loc blocks of locate_stride(K, 2) bytes, and a column blamed on two
// shards added into both shards' counts.
hipError_t launch_locate(ApplyArgs a, const LocateArgs& x, bool any_tail, hipStream_t stream,
                         LaunchEvents ev = {}, int max_errors = 1);

// ---- correct launches (rs_mixed.hip) -------------------------------------
// A locate launch that repairs what it blames: rs_apply_correct classifies a mismatching column
// with locate_correct and XORs the error value into the blamed shard's byte, through a.in_tab
// (whose shards must be writable) or a.out_tab. x as for launch_locate with max_errors 1;
// counts[stripe * nbins + shard] is the number of bytes of that shard the launch changed, bin
// nbins - 1 the columns left mismatching (with fewer than 3 compared rows: every mismatching
// column, and nothing is written).
// (kOrderCorrect + consecutive: rs_plan_forms of a correct plan)
constexpr int kOrderCorrect = 16384;
hipError_t launch_correct(ApplyArgs a, const LocateArgs& x, bool any_tail, hipStream_t stream,
                          LaunchEvents ev = {});

// Tiles per slice of a sliced launch (launch_apply's rule) for `streams` shard streams.
uint32_t launch_slice_tiles(int streams);

// Tuning hook for tools/kbench.hip (not part of the C ABI): tiles per launch slice for
// every later launch_apply in the process; 0 = never slice, < 0 = the built-in rule
// (CALLFS_RS_MAX_TILES_PER_LAUNCH or ~4 GiB of traffic per slice).
void set_slice_tiles_for_tuning(long long tiles);

}  // namespace callfs
