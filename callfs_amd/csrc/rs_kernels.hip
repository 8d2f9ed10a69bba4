// Kernel instantiations and launch dispatch for the RS path (device code in
// rs_apply.hpp). The production policy is chosen from tools/kbench.hip measurements
// on MI355X (DESIGN.md "Kernel tuning log").
#include <algorithm>
#include <array>
#include <atomic>
#include <cstdlib>
#include <mutex>
#include <optional>
#include <string>
#include <type_traits>
#include <utility>

#include <hip/hip_ext.h>

#include "bitslice.hpp"
#include "bitslice_rule.hpp"
#include "dispatch.hpp"
#include "launch_util.hpp"
#include "rs_apply.hpp"
#include "tile_order.hpp"
#include "tune_table.hpp"

namespace callfs {

namespace {

using dev::kBlock;
using O = TileOrder;

using VecFn = void (*)(ApplyArgs);
using ByteFn = void (*)(ApplyArgs, uint64_t);

// ---- kernel instances ---------------------------------------------------------------------
// Each kernel form is a policy template over (R, ORD) and a table of its instances indexed
// [TileOrder][R - R0], generated from the list of tile orders the form has instances for; an
// order without an instance holds null, and the form's fallback order is stated where the
// table is read (instance()).

// Policy::ORD of each TileOrder (tile_order.hpp map_tile, block_tile)
constexpr int kPolicyOrd[kTileOrders] = {0, 2, 5, 6, 8, 10, 11};
constexpr int policy_ord(TileOrder o) { return kPolicyOrd[static_cast<int>(o)]; }

template <int N>
using OrderTable = std::array<std::array<VecFn, N>, kTileOrders>;

// One tile order's row: policy P's instances for R = R0 .. R0 + N - 1 (kVecKernel: of the
// v_perm kernel, else of the LDS kernel). Every instance is checked here against the policy
// whose grid and tail placement (vec_grid, tail_code) its launches are computed for.
template <template <int, int> class P, class GridAs, bool kVecKernel, int R0, int ORD, int... Rs>
constexpr std::array<VecFn, sizeof...(Rs)> table_row(std::integer_sequence<int, Rs...>) {
  static_assert(((P<R0 + Rs, ORD>::BS == GridAs::BS && P<R0 + Rs, ORD>::TILE_VECS == GridAs::TILE_VECS) && ...),
                "one grid shape and tail placement for every policy of a kernel path");
  if constexpr (kVecKernel)
    return {&dev::rs_apply_vec<0, R0 + Rs, P<R0 + Rs, ORD>>...};
  else
    return {&dev::rs_apply_lds<R0 + Rs, P<R0 + Rs, ORD>>...};
}
template <template <int, int> class P, class GridAs, int R0, int N, bool kVecKernel, TileOrder... Os>
constexpr OrderTable<N> order_table() {
  OrderTable<N> t{};
  (..., (t[static_cast<int>(Os)] =
            table_row<P, GridAs, kVecKernel, R0, policy_ord(Os)>(std::make_integer_sequence<int, N>{})));
  return t;
}
template <template <int, int> class P, class GridAs, int R0, int N, TileOrder... Os>
constexpr OrderTable<N> lds_table() {
  return order_table<P, GridAs, R0, N, false, Os...>();
}
// ... of a form that only the A/B build has (every entry null in the product build)
template <template <int, int> class P, class GridAs, int R0, int N, TileOrder... Os>
constexpr OrderTable<N> ab_table() {
  if constexpr (kAbInstances)
    return order_table<P, GridAs, R0, N, false, Os...>();
  else
    return {};
}
// Entry [o][i] of a table, or the fallback order's where the form has no instance in o
template <size_t N>
VecFn instance(const std::array<std::array<VecFn, N>, kTileOrders>& t, TileOrder o, TileOrder fallback, int i) {
  const VecFn f = t[static_cast<int>(o)][i];
  return f ? f : t[static_cast<int>(fallback)][i];
}
#define CALLFS_EVERY_ORDER O::kConsecutive, O::kGroup8, O::kGroup2, O::kSeg8, O::kSeg16, O::kXcd8, O::kXcd32

// v_perm kernel policy (tools/kbench.hip on MI355X, RS(10,4) 1 MiB shards x 256 stripes,
// DESIGN.md "Kernel tuning log"): runtime-K pair loop, non-temporal loads and stores,
// 512-thread blocks, two input pairs in flight = 6118-6168 GB/s (76.5-77.1 % of
// 8 TB/s) vs 5457 GB/s for the first compile-time-K / plain-load version and
// 5957 GB/s for an XOR-only kernel with the same loads and stores. Used for k <= 3.
template <int R, int ORD>
using ProdOrderPolicy = dev::Policy<4, 1, true, true, false, 512, 2, ORD>;
using ProdPolicy = ProdOrderPolicy<1, 0>;
constexpr int kPermMaxRows = 4;  // v_perm kernel: k <= 3 and R <= 4 (takes_lds sends the rest to LDS)

// The LDS nibble-table kernel takes every launch with k >= 4 inputs or R >= 5 rows. Its
// cost per data byte barely grows with R, and with all 8 lookups of a dword in flight it
// also beats the v_perm kernel at R <= 4 (tools/kbench.hip, rotated order, 5 rounds,
// % of 8 TB/s): RS(10,4) 78.6 vs 73.0-75.7, RS(16,4) 77.4 vs 72.2-73.2, RS(20,4) 75.9
// vs 70.2-71.2, RS(4,2) 78.6 vs 76.6, RS(10,8) 71-72 vs 62, RS(32,8) 69.7 vs 49.3.
// With k <= 3 the per-block table prologue does not pay (RS(3,2): 73.3 vs 77.5-79.9),
// so those launches keep the v_perm kernel. One instance per R.
template <int R, int ORD>
using LdsRingPolicy = dev::Policy<2, 1, true, true, false, 512, 2, ORD>;
using LdsPolicy = LdsRingPolicy<1, 0>;
// Row groups of 9..16 (16-byte table entries, 100-127 VGPRs, 4 waves/SIMD): fewer waves
// hold fewer loads in flight, so they prefetch 4 input shards ahead through an unrolled
// 5-slot ring. RS(10,12) 61.5 -> 68.0 %, RS(10,16) 63.2 -> 69.3 %, RS(20,16) 59.3 ->
// 60.7 % of 8 TB/s (tools/kbench.hip, KB_RING). For R <= 8 the unrolled ring measured
// 1-3 % slower than the shifted ring of three, so those keep LdsPolicy.
// Their table addresses are formed by v_or_b32_sdwa (byte select + OR with an SGPR
// base) instead of v_perm_b32: same issue rate (tools/valu_rates.hip, 0.24 per SIMD
// clock), but no VGPR for the table base, which keeps R = 16 at 125 VGPRs (4 waves per
// SIMD; the v_perm form had grown to 129 = 3 waves once the ragged tail moved into the
// kernel). profiles/r02/sdwa/, % of 8 TB/s, v_perm -> SDWA:
// RS(10,16) 58.3 -> 66.8, RS(20,16) 52.2 -> 59.3, RS(32,16) 49.0 -> 55.0, RS(10,12)
// 65.9 -> 66.5.
template <int R, int ORD>
using LdsWideOrderPolicy = dev::Policy<2, 1, true, true, false, 512, 4, ORD, 1, false, false, true>;
using LdsWidePolicy = LdsWideOrderPolicy<9, 0>;
template <int R, int ORD>
using LdsPolicyFor =
    typename std::conditional<(R > 8), LdsWideOrderPolicy<R, ORD>, LdsRingPolicy<R, ORD>>::type;
// Launch groups of R <= 4 rows with Verify rows load the compared vectors 4 shards before
// the end of the input loop (rs_apply.hpp Policy::VPF):
// profiles/r02/verify_prefetch/, RS(10,4) 1 MiB x 256, % of 8 TB/s, after the loop ->
// prefetch distance 2 / 4 / 6 / 8: one write + three compare rows 71.6 -> 72.7 / 74.1 /
// 73.7 / 73.3, four compare rows 78.0 -> 79.3 / 80.9 / 80.8 / 79.5. Without Verify rows
// the same code measured 0.4 points slower (the extra registers), so encode launches keep
// the policies above: one instance per tile order.
template <int R, int ORD>
using LdsVerifyPolicy = dev::Policy<2, 1, true, true, false, 512, 2, ORD, 0, false, 0, false, 0, 4>;
// Misaligned shards (upstream Split layout of contiguous objects at odd S) with R <= 8:
// loads from aligned addresses realigned in registers, and parity stores to aligned
// addresses realigned the same way (62 vectors per wave; the bytes no aligned block
// covers are written by each stripe's first tile; rs_apply.hpp REALIGN 2). Round 1's
// form realigned only the loads (REALIGN 1, 63 vectors per wave, k >= 8; kept in
// tools/kbench for comparison). Round 2,
// profiles/r02/realign_out/, % of 8 TB/s, unaligned -> loads realigned -> loads and stores
// realigned: RS(10,4) 64 MiB objects (S = 6,710,887) 67.6 -> 68.1 -> 69.5, RS(10,8)
// 1,048,577 B 63.9 -> 65.3 -> 67.0, RS(6,3) 65.6 -> 67.0 -> 71.5, RS(5,3) 68.7 -> 66.7
// -> 72.2, RS(4,2) 69.0 -> 69.1 -> 69.8; RS(12,4) S = 5,592,406 ran 71.2 unaligned and
// 68.9 realigned, so rs_plan_tune offers the unaligned kernel as an alternative.
// (R <= 4 asks for 8 waves per SIMD: left alone the compiler used 106 SGPRs, 7 waves)
// One instance per tile order it runs in: consecutive, X8, X32 (tile_order.hpp block_tile).
template <int ORD>
using LdsRealignOutPolicy = dev::Policy<2, 1, true, true, false, 512, 2, ORD, 0, false, 2>;
template <int ORD>
using LdsRealignOut8Policy = dev::Policy<8, 1, true, true, false, 512, 2, ORD, 0, false, 2>;
template <int R, int ORD>
using LdsRealignOutPolicyFor =
    typename std::conditional<(R <= 4), LdsRealignOut8Policy<ORD>, LdsRealignOutPolicy<ORD>>::type;
using RealignGrid = LdsRealignOutPolicy<0>;  // 62-vector waves: the realigning forms' grid
static_assert(RealignGrid::BS == LdsPolicy::BS, "one block size for every LDS policy");
// R <= 4 with 6-bit lookups over shard triples (rs_apply.hpp Policy::WIX): 4 lookups per
// byte position of three shards instead of 6; one instance per tile order.
template <int R, int ORD>
using LdsWixPolicy = dev::Policy<8, 1, true, true, false, 512, 2, ORD, 0, false, 0, false, 0, 0, 1>;
// The triple loop with nibble lookups, R <= 8 (the rule's triple form, tile_order.hpp
// tri_rule_order; orders kOrderTri + TileOrder)
template <int R, int ORD>
using LdsTriPolicy = dev::Policy<(R <= 4 ? 8 : 2), 1, true, true, false, 512, 2, ORD, 0, false, 0, false, 0, 0, 2>;
// The triple loop with the Verify rows' compare loads issued with the triple that reaches
// K - 4 (Policy::VPF, as LdsVerifyPolicy): launches of R <= 4 rows that mix written and
// Verify rows (the one-erasure decode of a download) when they take triples
template <int R, int ORD>
using LdsTriVerifyPolicy = dev::Policy<2, 1, true, true, false, 512, 2, ORD, 0, false, 0, false, 0, 4, 2>;
// The triple loop double-buffered in two register sets with no conditional loads
// (rs_apply.hpp Policy::WIX 3): the compiler's waits then leave six loads in flight where
// the rotating form waited for the next triple inside each iteration. 81 VGPRs (5 waves
// per SIMD) at R <= 4; at R = 8 it needs 131 and lost (3 waves). Launches with R <= 4 and
// K >= 6 that take the triple form run it. profiles/r04/tridb/,
// % of 8 TB/s, rotating -> double-buffered triples in the same order: RS(10,4) 1 MiB 76.6
// -> 80.0 (G2), RS(8,4) 2 MiB 77.4 -> 80.5 (X32), RS(12,4) 1 MiB 79.4 -> 80.9 (G2),
// RS(6,3) 1 MiB 75.6 -> 78.4, 4 MiB 75.8 -> 78.1 (X32), RS(6,3) 174,763 B 72.2 -> 75.9,
// RS(10,4) 16 MiB 77.7 -> 77.9 (Q16); with K = 4 (no loop iteration) it lost 0.5-7 points.
template <int R, int ORD>
using LdsTriDbPolicy = dev::Policy<2, 1, true, true, false, 512, 2, ORD, 0, false, 0, false, 0, 0, 3>;
// ... with the Verify rows' compare loads issued with the last groups' loads (Policy::VPF):
// R <= 4 launches that mix written and Verify rows (one-erasure decodes), K >= 6; 92-96
// VGPRs at 5 waves per SIMD
template <int R, int ORD>
using LdsTriDbVerifyPolicy = dev::Policy<5, 1, true, true, false, 512, 2, ORD, 0, false, 0, false, 0, 4, 3>;
// The realigning kernel with its aligned loads issued in triples (rs_apply.hpp REALIGN
// with WIX 2)
template <int R, int ORD>
using LdsRealignTriPolicy =
    dev::Policy<(R <= 4 ? 7 : 2), 1, true, true, false, 512, 2, ORD, 0, false, 2, false, 0, 0, 2>;
// ... and the realigning kernel's aligned loads double-buffered in two triple sets
// (rs_apply.hpp WIX 3 with REALIGN 2), R <= 4 and K >= 6 (kTriDbMinK): A/B instances
// behind the realign-tri orders
template <int R, int ORD>
using LdsRealignTriDbPolicy = dev::Policy<5, 1, true, true, false, 512, 2, ORD, 0, false, 2, false, 0, 0, 3>;
// Misaligned inputs with 16-B-aligned outputs (upstream Split of an io.ReadAll body: the
// data shards inside the body, the parity in reedsolomon's AllocAligned buffers): 64-vector
// waves, lane 63's neighbour vector from one single-lane load per shard (rs_apply.hpp
// REALIGN 5), so the parity stores fill whole 1 KiB windows
// (A/B build; 512-vector tiles and the ragged tail as the plain kernel's)
template <int R, int ORD>
using LdsRealign64Policy =
    dev::Policy<6, 1, true, true, false, 512, 2, ORD, 0, false, 5>;
// Input vectors staged through an LDS-DMA ring of kDmaDepth shards per wave (rs_apply.hpp
// Policy::DMA): R <= 8, aligned shards, at most 64 KiB of LDS (K <= 64); A/B build
constexpr int kDmaDepth = 6;
template <int R, int ORD>
using LdsDmaPolicy = dev::Policy<(R <= 4 ? 8 : 6), 1, true, true, false, 512, 2, ORD, 0, false, 0,
                                 false, 0, 0, 0, kDmaDepth>;

// The instance tables, [TileOrder][R - R0], each from its policy and the orders it has instances
// for (in the order the kernels have always been emitted in, which kernel_resources.json lists).
#define CALLFS_TRI_ORDERS O::kConsecutive, O::kGroup2, O::kXcd32, O::kSeg8, O::kSeg16, O::kXcd8
#define CALLFS_REALIGN_ORDERS O::kConsecutive, O::kXcd8, O::kXcd32
// v_perm kernel, [consecutive, G2, Q16][R - 1]; any other order runs consecutive
const auto kVec = order_table<ProdOrderPolicy, ProdPolicy, 1, kPermMaxRows, true, O::kConsecutive,
                              O::kGroup2, O::kSeg16>();
// ring of three: [consecutive][R - 1] for every R, the other six orders for R <= 8 and
// [Q8][R - 9] for R 9..16 (any other order runs consecutive: ring_kernel); R <= 4 with Verify
// rows: every order
const auto kLds = lds_table<LdsPolicyFor, LdsPolicy, 1, kMaxRowsPerLaunch, O::kConsecutive>();
const auto kLdsRing = lds_table<LdsPolicyFor, LdsPolicy, 1, 8, O::kGroup8, O::kGroup2, O::kSeg8,
                                O::kSeg16, O::kXcd8, O::kXcd32>();
const auto kLdsVerify = lds_table<LdsVerifyPolicy, LdsPolicy, 1, 4, CALLFS_EVERY_ORDER>();
const auto kLdsWix = ab_table<LdsWixPolicy, LdsPolicy, 1, 4, CALLFS_EVERY_ORDER>();  // (A/B build)
// triples, [consecutive, G2, X32, Q8, Q16, X8][R - 1]: G8 has no triple instance and runs
// consecutive (tri_order maps the nibble rule's G8 to X32 before it gets here); the rotating
// early-compare form has no X8 instance either, which runs X32
const auto kLdsTri = lds_table<LdsTriPolicy, LdsPolicy, 1, 8, CALLFS_TRI_ORDERS>();
const auto kLdsTriDb = lds_table<LdsTriDbPolicy, LdsPolicy, 1, 4, CALLFS_TRI_ORDERS>();
const auto kLdsTriDbVerify = lds_table<LdsTriDbVerifyPolicy, LdsPolicy, 1, 4, CALLFS_TRI_ORDERS>();
const auto kLdsTriVerify = lds_table<LdsTriVerifyPolicy, LdsPolicy, 1, 4, O::kConsecutive, O::kGroup2,
                                     O::kXcd32, O::kSeg8, O::kSeg16>();
// LDS-DMA ring, [consecutive, G2, Q8, X32][R - 1]; any other order runs consecutive (A/B build)
const auto kLdsDma =
    ab_table<LdsDmaPolicy, LdsPolicy, 1, 8, O::kConsecutive, O::kGroup2, O::kSeg8, O::kXcd32>();
// [G4, G8][R - 1]: the double-buffered triples with 4 / 8 stripes interleaved (A/B build)
template <template <int, int> class P>
std::array<std::array<VecFn, 4>, 2> tridb_g_table() {
  if constexpr (kAbInstances)
    return {table_row<P, LdsPolicy, false, 1, 4>(std::make_integer_sequence<int, 4>{}),
            table_row<P, LdsPolicy, false, 1, 2>(std::make_integer_sequence<int, 4>{})};
  else
    return {};
}
const auto kLdsTriDbG = tridb_g_table<LdsTriDbPolicy>();
// realigning kernels, [consecutive, X8, X32][R - 1]; any other order runs X32 (realign_order)
const auto kLdsRealignTriDb = ab_table<LdsRealignTriDbPolicy, RealignGrid, 1, 4, CALLFS_REALIGN_ORDERS>();
const auto kLdsRealignTri = lds_table<LdsRealignTriPolicy, RealignGrid, 1, 8, CALLFS_REALIGN_ORDERS>();
const auto kLdsRealign64 = ab_table<LdsRealign64Policy, LdsPolicy, 1, 8, CALLFS_REALIGN_ORDERS>();
const auto kLdsRealignOut = lds_table<LdsRealignOutPolicyFor, RealignGrid, 1, 8, CALLFS_REALIGN_ORDERS>();
const auto kLdsWideQ8 = lds_table<LdsPolicyFor, LdsPolicy, 9, 8, O::kSeg8>();
VecFn ring_kernel(TileOrder o, int R) {
  const VecFn f = R <= 8 ? kLdsRing[static_cast<int>(o)][R - 1] : kLdsWideQ8[static_cast<int>(o)][R - 9];
  return f ? f : kLds[0][R - 1];
}

template <int... Rs>
constexpr auto byte_table(std::integer_sequence<int, Rs...>) {
  return std::array<ByteFn, sizeof...(Rs)>{&dev::rs_apply_bytes<Rs + 1>...};
}
const auto kByte = byte_table(std::make_integer_sequence<int, kMaxRowsPerLaunch>{});

// Row groups of 9..16 with more than 64 KiB of tables (k > 128) need the dynamic-LDS
// opt-in, which hipFuncSetAttribute sets for the current device only: one flag per
// (device, R), key R - 9 (dispatch.hpp DeviceOnce). Both tile-order instances of an R
// opt in together.
DeviceOnce g_wide_lds;

void wide_lds_opt_in(int R) {
  for (VecFn f : {ring_kernel(O::kConsecutive, R), ring_kernel(O::kSeg8, R)})
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(f),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 << 10);
}

// CALLFS_RS_TILE_ORDER=consecutive|g8|g2|q8|q16|x8|x32 overrides the rule for every LDS-kernel
// launch with R <= 8 (A/B on a deployment's own shard layout; unset = the rule).
std::optional<TileOrder> tile_order_override() {
  static const std::optional<TileOrder> v = []() -> std::optional<TileOrder> {
    const char* e = std::getenv("CALLFS_RS_TILE_ORDER");
    if (!e) return std::nullopt;
    static constexpr const char* kNames[kTileOrders] = {"consecutive", "g8", "g2", "q8", "q16", "x8", "x32"};
    static constexpr TileOrder kOrders[kTileOrders] = {CALLFS_EVERY_ORDER};
    for (int i = 0; i < kTileOrders; ++i)
      if (std::string(e) == kNames[i]) return kOrders[i];
    return std::nullopt;
  }();
  return v;
}
// An A/B toggle: CALLFS_RS_<name>=0 switches the form off, in the A/B build only
bool ab_toggle_on(const char* name) {
  const char* e = kAbInstances ? std::getenv(name) : nullptr;
  return !(e && *e == '0');
}
// CALLFS_RS_TRIDB=0 keeps R <= 4 triple launches on the rotating loop
bool tridb_enabled() {
  static const bool on = ab_toggle_on("CALLFS_RS_TRIDB");
  return on;
}
// CALLFS_RS_REALIGN=0 sends misaligned launches to the plain kernel (unaligned 16-B
// loads and stores)
bool realign_out_enabled() {
  static const bool on = ab_toggle_on("CALLFS_RS_REALIGN");
  return on;
}
// CALLFS_RS_WIX=0 keeps every launch on the ring-of-three nibble kernel
bool wix_enabled() {
  static const bool on = ab_toggle_on("CALLFS_RS_WIX");
  return on;
}
constexpr int kTriDbMinK = 6;

// What the rules and the kernel choice ask of a launch, computed once per call from its
// ApplyArgs (a.nvec and a.tail_in_vec are launch_apply's outputs and are not read).
struct Traits {
  uint64_t nvec;   // 16-byte vectors per shard
  uint64_t tps;    // tiles of 512 vectors (8 KiB) per stripe, the tile every rule counts in
  uint32_t rows;   // bit r set for each of the launch's R rows
  bool verify;     // some row is compared
  bool read_only;  // every row is compared (nothing is written)
  bool mixed;      // written and compared rows
  bool misaligned;
  explicit Traits(const ApplyArgs& a)
      : nvec(a.S / 16),
        tps((nvec + LdsPolicy::BS - 1) / LdsPolicy::BS),
        rows(a.R >= 32 ? ~0u : a.R > 0 ? (1u << a.R) - 1 : 0u),
        verify((a.verify_mask & rows) != 0),
        read_only((a.verify_mask & rows) == rows),
        mixed(verify && !read_only),
        misaligned((a.in_misalign | a.out_misalign) != 0) {}
};
static_assert(LdsPolicy::BS == 512 && LdsPolicy::TILE_VECS == 512 && ProdPolicy::TILE_VECS == 512 &&
                  bs::kTileVecs == 512,
              "one tile size for the rules (Traits::tps)");

// Tiles per kernel launch. Blocks are dealt to the 8 XCDs round-robin and each XCD runs
// its share in order, so over a long grid the XCDs drift apart and the tiles in flight
// spread over more of the address space than the tile order intends. Grids of more than
// twice about 4 GiB of shard traffic are cut into equal consecutive slices of at most
// that much (one launch each, same tile order), which resets the drift. Round 2 sweep
// (profiles/r02/slice_rule/, % of 8 TB/s, unsliced / 2 GiB /
// 4 GiB slices): RS(10,4) 64 MiB objects x 256 (24 GiB) 73.1 / 77.5 / 77.4, 1 MiB x 1,024
// 77.9 / 79.2 / 79.4, RS(4,2) 1 MiB x 2,048 76.8 / 79.2 / 79.3: long memory-bound grids
// need slices, and 4 GiB ones keep the gain. Every slice boundary drains the machine,
// which costs the grids of 4.5-12 GiB that 2 GiB slices used to cut: RS(10,8) 73.9 / 73.4
// / 74.0, RS(10,16) 69.3 / 68.0 / 69.2 (unsliced at 4 GiB), RS(20,4) 77.4 / 75.9 / 75.8
// (unsliced at 4 GiB), RS(32,8) 70.1 / 68.4 / 69.6, RS(32,16) 56.0 / 54.6 / 55.8; the
// bench grid (3.5 GiB) stays whole either way. CALLFS_RS_MAX_TILES_PER_LAUNCH sets the
// slice in tiles instead.
std::atomic<long long> g_slice_tiles_override{-1};

uint32_t slice_tiles(int streams) {
  static const long forced = [] {
    const char* e = std::getenv("CALLFS_RS_MAX_TILES_PER_LAUNCH");
    return e ? std::atol(e) : 0L;
  }();
  const long long ov = g_slice_tiles_override.load(std::memory_order_relaxed);
  if (ov == 0) return ~0u;  // never slice
  if (ov > 0) return static_cast<uint32_t>(std::min<long long>(std::max<long long>(ov, 1024), 1LL << 30));
  if (forced >= 1024) return static_cast<uint32_t>(std::min<long>(forced, 1L << 30));
  const uint64_t tile_bytes = 8192ull * static_cast<uint64_t>(std::max(1, streams));
  return static_cast<uint32_t>(std::max<uint64_t>(4096, (4ull << 30) / tile_bytes));
}

// Launches `grid` blocks of one kernel as consecutive slices (see slice_tiles). Launches
// that only compare (every row a Verify row, no stores) stay whole: read-only streams
// lose ≈ 1 point to the slice drains and gain nothing (configs[2] shape with nothing
// erased: 79.0-79.4 % whole vs 78.0-78.4 % sliced).
// launch(blocks, first, last): first / last = this is the launch's first / last slice.
template <class Launch>
void launch_sliced(uint32_t grid, ApplyArgs& a, const Traits& t, Launch&& launch) {
  launch_slices(grid, t.read_only ? grid : slice_tiles(a.K + a.R), a, launch);
}

// Ragged-tail placement (ApplyArgs::tail_in_vec, rs_apply.hpp tail_lane) for a kernel of
// TV-vector tiles and BS-thread blocks: the idle last wave of each stripe's last tile for
// stripes of at most kTailLastMaxTps tiles whose last tile leaves that wave idle, else wave
// 0 of the first tile. Round 4 moved every tail to the last tile (1 MiB-object shards, 7-22
// tiles per stripe, gained 0.4-1.3 points); on long stripes that put the grid's last tile
// behind the tail's load chain (profiles/r04/tail_ab: RS(20,4) S =
// 3,355,444, 410 tiles, first tile 73.8 %, last tile 72.6). CALLFS_RS_TAIL_LAST_TPS
// overrides the bound (A/B build only; clamped so that (tps - 1) << 2 fits the 32-bit code).
// Every LDS policy that takes this code tiles as LdsPolicy does (table_row's check); the
// realigning forms place their edges themselves (tail_in_vec = 1).
uint32_t tail_code(uint64_t nvec, uint64_t TV, uint64_t BS) {
  static const uint64_t max_tps = [] {
    const char* e = kAbInstances ? std::getenv("CALLFS_RS_TAIL_LAST_TPS") : nullptr;
    return std::min<uint64_t>(e && *e ? std::strtoull(e, nullptr, 10) : 32ull, 1ull << 29);
  }();
  const uint64_t tps = (nvec + TV - 1) / TV, last = nvec - (tps - 1) * TV;
  if (tps <= max_tps && last + 64 <= BS) return static_cast<uint32_t>(((tps - 1) << 2) | 3u);
  return 1u;
}

}  // namespace

namespace {
using SmallFn = void (*)(SmallArgs);
template <int... Rs>
constexpr auto small_table(std::integer_sequence<int, Rs...>) {
  return std::array<SmallFn, sizeof...(Rs)>{&dev::rs_apply_small<Rs + 1>...};
}
const auto kSmall = small_table(std::make_integer_sequence<int, kMaxRowsPerLaunch>{});
}  // namespace

hipError_t launch_small(const SmallArgs& a, hipStream_t stream) {
  if (a.R < 1 || a.R > kMaxRowsPerLaunch || a.K < 1 || a.K > kMaxK || a.batch < 1 ||
      a.batch > 65535 || a.nvec == 0 || !a.base || !a.tabs || !a.idx || !a.status)
    return hipErrorInvalidValue;
  const unsigned gx = (a.nvec + 255u) / 256u;
  hipLaunchKernelGGL(kSmall[a.R - 1], dim3(gx, static_cast<unsigned>(a.batch)), dim3(256), 0,
                     stream, a);
  return hipGetLastError();
}

namespace {
using SmallRaggedFn = void (*)(SmallRaggedArgs);
template <int... Rs>
constexpr auto small_ragged_table(std::integer_sequence<int, Rs...>) {
  return std::array<SmallRaggedFn, sizeof...(Rs)>{&dev::rs_apply_small_ragged<Rs + 1>...};
}
const auto kSmallRagged = small_ragged_table(std::make_integer_sequence<int, kMaxRowsPerLaunch>{});
}  // namespace

hipError_t launch_small_ragged(const SmallRaggedArgs& a, hipStream_t stream) {
  if (a.R < 1 || a.R > kMaxRowsPerLaunch || a.K < 1 || a.K > kMaxK || a.nitems < 1 ||
      a.nitems > 65535 || a.max_nvec == 0 || a.row0 < 0 || !a.base || !a.items || !a.ptabs ||
      !a.status || !a.counter)
    return hipErrorInvalidValue;
  const unsigned gx = (a.max_nvec + 255u) / 256u;
  hipLaunchKernelGGL(kSmallRagged[a.R - 1], dim3(gx, static_cast<unsigned>(a.nitems)), dim3(256), 0,
                     stream, a);
  return hipGetLastError();
}

void set_slice_tiles_for_tuning(long long tiles) {
  g_slice_tiles_override.store(tiles, std::memory_order_relaxed);
}

uint32_t launch_slice_tiles(int streams) { return slice_tiles(streams); }

namespace {

constexpr int kLdsMinRows = 5;
constexpr int kLdsMinK = 4;

TileOrder lds_rule(const ApplyArgs& a, const Traits& t) {
  if (const auto forced = tile_order_override()) return *forced;
  return lds_tile_order(a.S, t.tps, a.addr_tz, a.K + a.R, a.stripe_stride, t.verify, t.read_only, a.R);
}
TileOrder wide_rule(const Traits& t) { return wide_tile_order(t.tps); }
TileOrder vec_rule(const ApplyArgs& a, const Traits& t) { return vec_tile_order(a.S, t.tps, a.addr_tz); }

bool takes_lds(const ApplyArgs& a) { return a.R >= kLdsMinRows || a.K >= kLdsMinK; }
// Misaligned R <= 8 launches can take the realigning kernel; by default they do when some
// shard sits at an odd byte offset. Shards misaligned only by even offsets (even S) ran
// the plain kernel 2.3-4.3 points faster (RS(12,4), S = 5,592,406, two boxes), odd ones
// mostly slower (RS(6,3) -6, RS(5,3) -4, RS(10,8) -1.7; RS(10,4) and RS(4,2) within
// +-1.4 depending on the box). rs_plan_tune times both.
bool can_realign(const ApplyArgs& a, const Traits& t) {
  return a.R <= 8 && t.misaligned && realign_out_enabled();
}
// 6-bit triple lookups (Policy::WIX): R <= 4, 3 <= K <= 96 (tables within the 64 KiB of
// dynamic LDS a launch gets without the opt-in), aligned shards
bool can_wix(const ApplyArgs& a, const Traits& t) {
  return kAbInstances && a.R <= 4 && a.K >= 3 && a.K <= 96 && !t.misaligned;
}
bool can_tridb_g(const ApplyArgs& a, const Traits& t) {
  return kAbInstances && a.R <= 4 && a.K >= kTriDbMinK && !t.misaligned && !t.verify;
}
bool can_dma(const ApplyArgs& a, const Traits& t) {
  return kAbInstances && a.R <= 8 && a.K >= 2 && !t.misaligned &&
         dev::lds_bytes_dma(a.K, a.R, kDmaDepth) <= (64u << 10);
}
// the 64-vector realigning form: misaligned inputs, every output 16-B aligned
bool can_realign64(const ApplyArgs& a, const Traits& t) {
  return kAbInstances && can_realign(a, t) && a.in_misalign && !a.out_misalign;
}
// Since the triple-load form (below) measured equal or faster than WIX everywhere, the
// rule no longer takes WIX: its instances remain for rs_plan_set_orders (A/B).
// profiles/r03/wix/: WIX in the nibble rule's order vs the nibble kernel's best order, 1 MiB shards: RS(4,2) 72.3 -> 79.0, RS(4,4) 75.0 -> 81.5, RS(5,3) 74.5 -> 79.9,
// RS(8,4) 76.5 -> 80.1; RS(10,4) equal, RS(16,4) / RS(20,4) / RS(32,4) -1.2 ... -1.5.

// Triple loads (Policy::WIX 2): tile_order.hpp tri_rule. profiles/r03/wix/ab4_tri_verify.jsonl, % of 8 TB/s, nibble (best order) -> triples in
// the rule's order: RS(4,2) 71.8 -> 80.6, RS(5,3) 74.6 -> 80.3, RS(8,4) 76.3 -> 80.2,
// RS(10,4) 75.8 -> 76.6, RS(6,6) 74.6 -> 75.7, RS(8,8) 75.4 -> 76.3, RS(10,8) 74.1 -> 77.4;
// read-only (download Verify): RS(4,2) 82.5 -> 88.4, RS(10,4) 83.8 -> 86.0 (X32). Second
// box (profiles/r03/tri1/ab.jsonl), the rule itself: RS(4,2) 72.5 -> 80.6, 1 MiB objects
// 71.9 -> 77.9, RS(8,8) 75.6 -> 77.6, RS(10,8) 74.4 -> 78.2, RS(4,2) read-only 82.8 ->
// 88.0, RS(6,3) 1 MiB objects 71.4 -> 73.2, RS(10,4) 76.5 -> 75.9-76.1 (the tuner keeps
// whichever is faster), RS(12,4) 77.2 -> 80.3 (G2).
// The rule's triple-form order (tile_order.hpp tri_rule_order: round 4 adds X32 for K <= 4,
// X32 / Q16 for K 5..6 and Q16 on 16-32 MiB power-of-two pitches), or -1. With
// CALLFS_RS_TILE_ORDER set, the triple form follows the forced order with round 3's bounds.
// Misaligned inputs with 16-B-aligned outputs (upstream Split of an io.ReadAll body: the
// data shards inside the body, the parity in AllocAligned buffers): the triple form with
// unaligned 16-B loads, X32 up to 256 tiles per stripe and X8 above, not the realigning
// kernel. profiles/r04/utri1/readall_enc.jsonl (% of 8 TB/s,
// realigning kernel (rule) -> triples in X32 / X8): RS(10,4) 104,858 B 69.5 -> 76.7 (G2
// 77.5), RS(12,4) 87,382 B 69.0 -> 75.7, RS(5,3) 209,716 B 71.0 -> 78.3, RS(6,3) 174,763 B
// 70.6 -> 74.4, RS(10,8) 1,048,577 B 68.8 -> 70.9, RS(10,4) 6,710,887 B 71.2 -> 72.8 (X8),
// RS(12,4) 5,592,406 B 71.8 -> 74.2 (X8), RS(4,2) 1,048,577 B 71.0 -> 71.9. With unaligned
// stores as well (the contiguous Split layout) the same forms lost 1-6 points
// (split_enc.jsonl), so misaligned outputs keep the realigning kernel.
// (Measured for K <= 12 only; wider launches above 256 KiB shards keep the realigning
// kernel, as the aligned rule keeps K > 12 off the triples there.)
std::optional<TileOrder> tri_unaligned_order(const ApplyArgs& a, const Traits& t) {
  if (a.R > 8 || a.K < 4 || !a.in_misalign || a.out_misalign || tile_order_override())
    return std::nullopt;
  // More than 12 inputs above 256 KiB: the realigning ring, except for R <= 4 launches that
  // also compare rows (one-shard decodes), where the unaligned triples lead it (round 5, 40
  // seeded object sizes in the readall layout, profiles/r05/tiles/random_readall_*: RS(16,4)
  // 2.3 MB decode {1} 70.9 -> 73.6; its encodes split, 3.9 MB 73.4 -> 69.9)
  if (a.K > 12 && t.tps > 32 && !(a.R <= 4 && t.verify)) return std::nullopt;
  // R 5..8 launches that compare rows take a ring, as the aligned rule gives them the ring
  // (the plain one on unaligned loads, takes_realign): the rotating unaligned triples ran
  // 3-7 points behind the ring forms (RS(8,8) /
  // RS(10,8) {1}, 122 KB - 24 MB: 62-64 vs 65.7-71.0; after: those 8 cells 63.7 -> 66.4
  // on average, random_readall_dec1_after.jsonl)
  if (a.R > 4 && t.verify) return std::nullopt;
  // round 5 (tools/jobs.sh readall_rule_sweep, profiles/r05/readall_rule/): Q8 from 1 to 2 MiB,
  // X32 -> Q8: RS(10,4) 1.68 MB 74.9 -> 76.6, RS(12,4) 1.4 MB 75.1 -> 76.3, RS(8,8) 2 MiB
  // 75.0 -> 76.3, RS(10,8) 1.68 MB 70.4 -> 71.7
  if (t.tps > 128 && t.tps <= 256) return TileOrder::kSeg8;
  return t.tps <= 256 ? TileOrder::kXcd32 : TileOrder::kXcd8;
}

// The triple form's tile order when the rule takes it for this launch
std::optional<TileOrder> tri_rule_of(const ApplyArgs& a, const Traits& t) {
  if (!wix_enabled() || !takes_lds(a)) return std::nullopt;
  if (a.in_misalign && !a.out_misalign) return tri_unaligned_order(a, t);
  if (tile_order_override()) {
    if (tri_rule(a.K, a.R, t.misaligned, t.verify, t.read_only, t.tps) &&
        (t.tps <= 256 || (t.tps <= 512 && a.K <= 6)))
      return tri_order(lds_rule(a, t));
    return std::nullopt;
  }
  // (tri_rule_order's int: a TileOrder's value, or -1)
  static constexpr TileOrder kOrders[kTileOrders] = {CALLFS_EVERY_ORDER};
  const int o = tri_rule_order(a.K, a.R, t.misaligned, t.verify, t.read_only, t.tps, a.addr_tz, a.S,
                               lds_rule(a, t));
  return o < 0 ? std::nullopt : std::optional<TileOrder>(kOrders[o]);
}
bool tri_tunable_launch(const ApplyArgs& a, const Traits& t) {
  return wix_enabled() && tri_tunable(a.K, a.R, t.misaligned, t.verify, t.read_only);
}
bool takes_realign(const ApplyArgs& a, const Traits& t) {
  // (round 5: R 5..8 launches with misaligned inputs, aligned outputs and compared rows run
  // the plain ring on unaligned loads 3.2-4.5 points ahead of the realigning form, RS(8,8)
  // 23.8 MB {1} readall 67.8 -> 72.3, RS(10,8) 161,009 B 62.1 -> 66.6;
  // profiles/r05/tiles/random_readall_dec1_after.jsonl)
  if (a.R > 4 && t.verify && a.in_misalign && !a.out_misalign) return false;
  return can_realign(a, t) && ((a.in_misalign | a.out_misalign) & 1u) && !tri_rule_of(a, t);
}

// The rule's realigning launches with triple loads (tile_order.hpp realign_tri_rule);
// CALLFS_RS_WIX=0 keeps them on the ring of three
bool takes_realign_tri(const ApplyArgs& a, const Traits& t) {
  return wix_enabled() && realign_tri_rule(a.K, a.R, t.verify, t.read_only);
}

// The realigning kernels' tile order (instances: consecutive, X8, X32): the one a realigning
// code names, for the rule CALLFS_RS_TILE_ORDER's; any other, or none, runs X32 (DESIGN.md
// §6.2: tools/order_ab.py, Split
// layout, % of 8 TB/s, two runs, consecutive -> X32: RS(10,4) 64 MiB objects 68.3 /
// 68.6 -> 69.5 / 69.9, RS(4,2) 1,048,577 B 67.1 / 66.8 -> 68.6 / 68.3, RS(12,4) S =
// 5,592,406 65.5 / 65.9 -> 66.9 / 66.9, the other five shapes -0.2 ... +0.9).
TileOrder realign_order(Form f) {
  const std::optional<TileOrder> o = f.family == Family::kRule ? tile_order_override()
                                     : f.has_order()           ? std::optional<TileOrder>(f.order())
                                                               : std::nullopt;
  return o == TileOrder::kConsecutive || o == TileOrder::kXcd8 ? *o : TileOrder::kXcd32;
}

// The bit-sliced kernel's orders: launch groups of kBitsliceMinRows or more
// rows whose plan carries a kernel handle (ApplyArgs::bs), unless CALLFS_RS_BITSLICE=0.
bool can_bitslice(const ApplyArgs& a) {
  return a.bs && a.R >= kBitsliceMinRows && a.K >= 1 && a.S >= 16 && bs::mode() != bs::Mode::kOff;
}
// The rule's bit-sliced launches and their order (tile_order.hpp bitslice_rule)
bool takes_bitslice(const ApplyArgs& a, const Traits& t) {
  return can_bitslice(a) &&
         bitslice_rule(a.K, a.R, t.tps, a.in_misalign != 0, a.out_misalign != 0, t.verify, t.read_only);
}
TileOrder bitslice_rule_order(const Traits& t) {
  return bitslice_tile_order(t.tps, t.misaligned, t.verify, t.read_only);
}
// bs::Args::order of each TileOrder
constexpr int kBitsliceOrder[kTileOrders] = {0, 5, 3, 1, 6, 4, 2};

TuneKey key_of(const ApplyArgs& a, const Traits& t) {
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) device = 0;
  return tune_key(device, a.K, a.R, t.tps, a.addr_tz, t.verify, t.read_only, a.in_misalign != 0,
                  a.out_misalign != 0);
}

using Forms = std::vector<Form>;
void add(Forms& c, Form f) {
  if (std::find(c.begin(), c.end(), f) == c.end()) c.push_back(f);
}

// The nibble-table and v_perm forms worth timing (order_candidates without the bit-sliced ones)
Forms nibble_candidates(const ApplyArgs& a, const Traits& t, bool every_instance) {
  Forms c;
  const auto plain = [&c](TileOrder o) { add(c, form_of(Family::kPlain, o)); };
  const auto tri = [&c](TileOrder o) { add(c, form_of(Family::kTri, o)); };
  const auto in = [&c](Family f, std::initializer_list<TileOrder> os) {
    for (TileOrder o : os) add(c, form_of(f, o));
  };
  if (t.nvec == 0 || a.R < 1 || a.R > kMaxRowsPerLaunch || a.K < 1) return c;
  const uint64_t tps = t.tps;
  if (!takes_lds(a)) {
    plain(vec_rule(a, t));
    plain(O::kConsecutive);
    plain(O::kGroup2);
    if (tps > 1024) plain(O::kSeg16);
    return c;
  }
  if (a.R > 8) {
    plain(wide_rule(t));
    plain(O::kConsecutive);
    plain(O::kSeg8);
    return c;
  }
  // the rule's kernel first (rs_plan_tune's bar favours cand[0]): the realign order the
  // rule itself runs (realign_order follows CALLFS_RS_TILE_ORDER)
  if (takes_realign(a, t)) add(c, form_of(Family::kRealign, realign_order(Form{})));
  if (const auto o = tri_rule_of(a, t)) tri(*o);  // the rule's kernel first
  plain(lds_rule(a, t));
  if (can_realign(a, t)) {
    in(Family::kRealign, {O::kXcd32, O::kConsecutive});
    if (every_instance) in(Family::kRealign, {O::kXcd8});
    if (every_instance && can_realign64(a, t))  // (A/B build)
      in(Family::kRealign64, {O::kXcd32, O::kConsecutive, O::kXcd8});
    if (a.K >= 3) {  // the realigning kernel with triple loads
      in(Family::kRealignTri, {O::kXcd32, O::kConsecutive});
      if (every_instance) in(Family::kRealignTri, {O::kXcd8});
    }
  }
  plain(O::kConsecutive);
  plain(O::kGroup2);
  if (tps <= 32 || every_instance) plain(O::kGroup8);
  // Q8 from 64 tiles per stripe (8 segments of >= 8 tiles): at 1 MiB shards it ran within
  // a point of the best order and ahead of the rule's on some boxes (RS(16,4) 77.7 vs 76.8,
  // profiles/r04/tri_sweep1); Q16 above 8 MiB as before
  if (tps >= 64) plain(O::kSeg8);
  if (tps > 1024 || (every_instance && tps >= 64)) plain(O::kSeg16);
  if (every_instance) {  // on aligned shards never faster than the rule's order, which
                         // is X32 itself for read-only launches
    plain(O::kXcd8);
    plain(O::kXcd32);
  }
  // (on misaligned shards the triple forms are the plain kernel's unaligned 16-B
  // accesses: A/B instances for rs_plan_set_orders)
  // (misaligned launches: the tuner also times the triple forms' unaligned accesses,
  // which the rule takes for aligned outputs only)
  if ((every_instance && a.K >= 3) || tri_tunable_launch(a, t) ||
      (a.in_misalign && a.R <= 8 && a.K >= 4 && wix_enabled())) {
    in(Family::kTri, {O::kConsecutive, O::kGroup2, O::kXcd32});
    // tri-Q8 from 64 tiles per stripe (RS(10,4) 1 MiB 77.5 / 77.3 against 76.3 / 76.2 for
    // tri-G2, profiles/r04/tri_sweep1, tri_sweep2); tri-Q16 above 8 MiB
    if (tps >= 64) tri(O::kSeg8);
    if (tps > 1024 || (every_instance && tps >= 64)) tri(O::kSeg16);
    if (tps > 1024 || every_instance) tri(O::kXcd8);
  }
  if (every_instance && can_tridb_g(a, t)) {  // G4 / G8 double-buffered triples: A/B build only
    add(c, Form{Family::kTriDbG, 0});
    add(c, Form{Family::kTriDbG, 1});
  }
  if (every_instance && can_dma(a, t))  // the LDS-DMA ring: A/B build only
    in(Family::kDma, {O::kConsecutive, O::kGroup2, O::kSeg8, O::kXcd32});
  if (every_instance && can_wix(a, t)) {  // WIX in every plain order offered: A/B build only
    const size_t n0 = c.size();
    for (size_t i = 0; i < n0; ++i)
      if (c[i].family == Family::kPlain) add(c, Form{Family::kWix, c[i].member});
  }
  return c;
}

Forms candidates(const ApplyArgs& a, const Traits& t, bool every_instance) {
  Forms c = nibble_candidates(a, t, every_instance);
  if (c.empty()) return c;
  // the rule's kernel first (rs_plan_tune's bar favours cand[0])
  if (takes_bitslice(a, t)) c.insert(c.begin(), form_of(Family::kBitslice, bitslice_rule_order(t)));
  if (can_bitslice(a)) {
    const auto bs = [&c](TileOrder o) { add(c, form_of(Family::kBitslice, o)); };
    bs(bitslice_rule_order(t));
    bs(O::kConsecutive);
    bs(O::kGroup2);
    if (t.tps <= 32 || every_instance) bs(O::kGroup8);
    if (t.tps >= 64 || every_instance) bs(O::kSeg8);
    if (t.tps >= 256 || every_instance) bs(O::kSeg16);
    if (every_instance) {
      bs(O::kXcd8);
      bs(O::kXcd32);
    }
  }
  return c;
}

}  // namespace

bool bitslice_wanted(const ApplyArgs& a) { return takes_bitslice(a, Traits(a)); }

std::vector<int> order_candidates(const ApplyArgs& a, bool every_instance) {
  std::vector<int> codes;
  for (Form f : candidates(a, Traits(a), every_instance)) codes.push_back(encode(f));
  return codes;
}

int tuned_order(const ApplyArgs& a) {
  TuneTable& tab = tune_table();
  if (tab.empty()) return -1;
  const Traits t(a);
  const int o = tab.lookup(key_of(a, t));
  if (o < 0) return -1;
  const Form f = decode_order(o);
  const Forms c = candidates(a, t, /*every_instance=*/true);
  if (!f.valid() || std::find(c.begin(), c.end(), f) == c.end()) return -1;
  if (f.family == Family::kBitslice) {  // host calls never wait for a compile: the rule until it is ready
    auto* k = static_cast<bs::Kernel*>(const_cast<void*>(a.bs));
    if (k->state() != bs::Kernel::State::kReady) {
      k->compile_async();
      return -1;
    }
  }
  return o;
}

void record_tuned(const ApplyArgs& a, int order) { tune_table().record(key_of(a, Traits(a)), order); }

int launch_form(const ApplyArgs& a, int order) {
  if (decode_order(order).family == Family::kRule) order = tuned_order(a);
  if (decode_order(order).family != Family::kRule) return order;
  const Traits t(a);
  if (takes_bitslice(a, t) && static_cast<const bs::Kernel*>(a.bs)->state() == bs::Kernel::State::kReady)
    return encode(form_of(Family::kBitslice, bitslice_rule_order(t)));
  const Forms c = nibble_candidates(a, t, false);
  return c.empty() ? -1 : encode(c[0]);
}

namespace {
// One launch of the group's bit-sliced kernel in tile order `ord` (plus the byte kernel for
// the S % 16 tail). Returns false, launching nothing, when the kernel is not compiled yet and
// `wait` is false (the caller then runs the nibble-table kernel); with `wait` a kernel that
// cannot be compiled or loaded returns true with *err set.
bool launch_bitslice(ApplyArgs a, const Traits& t, hipStream_t stream, TileOrder ord, LaunchEvents ev,
                     bool wait, hipError_t* err) {
  *err = hipSuccess;
  if (!can_bitslice(a)) {
    if (wait) *err = hipErrorInvalidValue;
    return wait;
  }
  int device = -1;
  if (hipGetDevice(&device) != hipSuccess) {
    *err = hipErrorInvalidDevice;
    return true;
  }
  auto* k = static_cast<bs::Kernel*>(const_cast<void*>(a.bs));
  const hipFunction_t fn = k->function(device, wait);
  if (!fn) {
    if (wait) *err = hipErrorNoBinaryForGpu;
    return wait;
  }
  bs::Args b{};
  b.in_tab = a.in_tab;
  b.out_tab = a.out_tab;
  b.status = a.status;
  b.nvec = a.S / 16;
  b.tps = static_cast<uint32_t>((b.nvec + k->tile_vecs() - 1) / k->tile_vecs());
  b.ntiles = b.tps * static_cast<uint32_t>(a.batch);
  b.verify_mask = a.verify_mask;
  b.status_stride = a.status_stride;
  b.order = kBitsliceOrder[static_cast<int>(ord)];
  const bool tail_after = b.nvec * 16 < a.S;
  launch_sliced(b.ntiles, a, t, [&](uint32_t blocks, bool first, bool last) {
    b.t_base = a.t_base;
    const hipError_t e = bs::launch(fn, b, blocks, k->block_threads(), stream,
                                    first ? ev.start : nullptr, last && !tail_after ? ev.stop : nullptr);
    if (e != hipSuccess && *err == hipSuccess) *err = e;
  });
  if (*err != hipSuccess) return true;
  if (tail_after) {
    const uint64_t tail0 = b.nvec * 16;
    const unsigned gy = static_cast<unsigned>(std::min(a.batch, 65535));
    const uint64_t gx = (a.S - tail0 + kBlock - 1) / kBlock;
    dispatch(kByte[a.R - 1], dim3(static_cast<unsigned>(gx), gy), dim3(kBlock), 0, stream, ev,
             /*first=*/false, /*last=*/true, a, tail0);
    *err = hipGetLastError();
  }
  return true;
}

// What one vector-kernel launch runs: the kernel, its dynamic LDS bytes, grid and block, where
// the S % 16 tail goes (ApplyArgs::tail_in_vec; tail0 = the first byte left to the byte
// kernel, S when there is none) and whether the kernel needs the wide-LDS opt-in first.
// fn = null: the launch lacks the tables its kernel reads.
struct Selection {
  VecFn fn = nullptr;
  size_t lds = 0;
  unsigned grid = 0;
  int block = 0;
  uint32_t tail_in_vec = 0;
  uint64_t tail0 = 0;
  bool wide_lds = false;
};

bool realigning(Form f) {
  return f.family == Family::kRealign || f.family == Family::kRealignTri || f.family == Family::kRealign64;
}

// A code whose form this launch cannot take runs the rule instead; WIX without its instances
// runs the nibble kernel in the same order.
Form feasible(const ApplyArgs& a, const Traits& t, Form f) {
  switch (f.family) {
    case Family::kTriDbG: return can_tridb_g(a, t) && f.has_order() ? f : Form{};
    case Family::kDma: return can_dma(a, t) ? f : Form{};
    case Family::kRealign64: return can_realign64(a, t) ? f : Form{};
    case Family::kRealignTri: return a.K >= 3 && can_realign(a, t) ? f : Form{};
    case Family::kTri: return a.R <= 8 && a.K >= 3 ? f : Form{};
    case Family::kWix: return can_wix(a, t) ? f : Form{Family::kPlain, f.member};
    default: return f;
  }
}

// The tile order a code names for the kernels in the aligned kernels' orders (none: the rule,
// a realigning code, or a code past its family's members)
std::optional<TileOrder> named_order(Form f) {
  return f.family == Family::kRule || realigning(f) || !f.has_order() ? std::nullopt
                                                                     : std::optional<TileOrder>(f.order());
}

// The triple-loop instance for tile order o: rotating, or with R <= 4 and K >= kTriDbMinK
// double-buffered; launches of R <= 4 rows that mix written and Verify rows take the forms
// with early compare loads
VecFn tri_kernel(const ApplyArgs& a, const Traits& t, TileOrder o) {
  const int i = a.R - 1;
  const bool db = a.K >= kTriDbMinK && tridb_enabled();
  if (a.R <= 4 && t.mixed) {
    if (db) return instance(kLdsTriDbVerify, o, O::kConsecutive, i);
    return instance(kLdsTriVerify, o == O::kGroup8 ? O::kConsecutive : o, O::kXcd32, i);
  }
  if (a.R <= 4 && db) return instance(kLdsTriDb, o, O::kConsecutive, i);
  return instance(kLdsTri, o, O::kConsecutive, i);
}

// The vector kernel of launch `a` for form f (a decoded order code; Form{} = the rule).
// a.nvec = t.nvec > 0.
Selection select_kernel(const ApplyArgs& a, const Traits& t, Form f) {
  f = feasible(a, t, f);
  const bool by_rule = f.family == Family::kRule, tail = t.nvec * 16 < a.S;
  const std::optional<TileOrder> named = named_order(f);
  const int i = a.R - 1;
  Selection s;
  static_assert(ProdPolicy::BS == LdsPolicy::BS, "one block size for both kernel paths");
  s.block = LdsPolicy::BS;
  // the first tile per stripe computes the S % 16 tail itself: an odd-S launch (Split layout)
  // is one kernel, not two back to back
  s.tail_in_vec = tail ? tail_code(t.nvec, LdsPolicy::TILE_VECS, LdsPolicy::BS) : 0u;
  s.tail0 = s.tail_in_vec ? a.S : t.nvec * 16;
  s.grid = dev::vec_grid<LdsPolicy>(t.nvec, a.batch);
  if (!takes_lds(a)) {  // R <= 4 here (R >= kLdsMinRows takes the LDS kernel)
    const TileOrder ord = by_rule ? vec_rule(a, t) : named.value_or(O::kConsecutive);
    s.fn = instance(kVec, ord, O::kConsecutive, i);
    return s;
  }
  if (!a.ltabs) return s;
  s.lds = dev::lds_bytes(a.K, a.R);
  if (a.R > 8) {
    // more than 64 KiB of 16-byte entries (K > 128) needs the opt-in; R <= 8 never does
    // (8-byte entries, and the WIX and DMA forms are bounded by can_wix / can_dma)
    s.wide_lds = s.lds > (64u << 10);
    const TileOrder ord = by_rule ? wide_rule(t) : named.value_or(O::kConsecutive);
    s.fn = ring_kernel(ord, a.R);
    return s;
  }
  // misaligned shards: the realigning form, unless a tuned order names a plain kernel
  if (f.family == Family::kRealign64) {
    s.fn = kLdsRealign64[static_cast<int>(realign_order(f))][i];
    return s;
  }
  if (can_realign(a, t) && (realigning(f) || (by_rule && takes_realign(a, t)))) {
    const bool tri = f.family == Family::kRealignTri || (by_rule && takes_realign_tri(a, t));
    const int o = static_cast<int>(realign_order(f));
    if (!tri)
      s.fn = kLdsRealignOut[o][i];
    else if (kAbInstances && a.R <= 4 && a.K >= kTriDbMinK && tridb_enabled())
      s.fn = kLdsRealignTriDb[o][i];
    else
      s.fn = kLdsRealignTri[o][i];
    s.grid = dev::vec_grid<RealignGrid>(t.nvec, a.batch);
    s.tail_in_vec = 1;  // its first tile writes every edge byte, the tail included
    s.tail0 = a.S;
    return s;
  }
  // The aligned kernels, in the code's order or else the nibble rule's. A code past its
  // family's members runs the family's consecutive instance, the ring without the Verify
  // rows' early loads.
  const bool unknown = !by_rule && !realigning(f) && !named;
  const TileOrder ord = named ? *named : unknown ? O::kConsecutive : lds_rule(a, t);
  const int o = static_cast<int>(ord);
  const std::optional<TileOrder> rule_tri = by_rule ? tri_rule_of(a, t) : std::nullopt;
  if (f.family == Family::kTri || rule_tri) {
    s.fn = tri_kernel(a, t, rule_tri ? *rule_tri : ord);
  } else if (f.family == Family::kTriDbG) {  // (the nibble instances' G8 order underneath)
    s.fn = kLdsTriDbG[f.member][i];
  } else if (f.family == Family::kDma) {
    s.fn = instance(kLdsDma, ord, O::kConsecutive, i);
    s.lds = dev::lds_bytes_dma(a.K, a.R, kDmaDepth);
  } else if (f.family == Family::kWix && !unknown) {  // (at most 56 KiB of tables at K = 96)
    s.fn = kLdsWix[o][i];
    s.lds = dev::lds_bytes_wix(a.K);
  } else {
    s.fn = a.R <= 4 && t.verify && !unknown ? kLdsVerify[o][i] : ring_kernel(ord, a.R);
  }
  return s;
}

}  // namespace

hipError_t launch_apply(ApplyArgs a, hipStream_t stream, bool bytes_only, int order,
                        LaunchEvents ev) {
  if (a.R < 1 || a.R > kMaxRowsPerLaunch || a.K < 1 || a.K > kMaxK || a.batch < 1)
    return hipErrorInvalidValue;
  if (a.S == 0) return hipSuccess;
  const Traits t(a);
  Form f = decode_order(order);
  // the bit-sliced kernel: a pinned kOrderBitslice order waits for its compile; the rule's
  // choice runs it once compiled and the nibble-table kernel until then
  if (!bytes_only && (f.family == Family::kBitslice || (f.family == Family::kRule && takes_bitslice(a, t)))) {
    const bool pinned = f.family == Family::kBitslice;
    if (pinned && !f.has_order()) return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    if (launch_bitslice(a, t, stream, pinned ? f.order() : bitslice_rule_order(t), ev,
                        pinned || bs::mode() == bs::Mode::kSync, &e))
      return e;
    f = Form{};
  }
  a.nvec = bytes_only ? 0 : t.nvec;
  a.tail_in_vec = 0;
  uint64_t tail0 = 0;
  if (a.nvec) {
    const Selection s = select_kernel(a, t, f);
    if (!s.fn) return hipErrorInvalidValue;
    if (s.wide_lds) {
      // the opt-in is a per-device attribute: once per (device, R), before the first
      // such launch on each device (a once-flag per kernel left devices 1..7 without it)
      int device = -1;
      if (hipGetDevice(&device) != hipSuccess) return hipErrorInvalidDevice;
      g_wide_lds.run(device, a.R - 9, [&a] { wide_lds_opt_in(a.R); });
    }
    a.tail_in_vec = s.tail_in_vec;
    tail0 = s.tail0;
    const bool tail_after = tail0 < a.S;  // a byte-kernel launch follows: it ends the launch
    launch_sliced(s.grid, a, t, [&](uint32_t blocks, bool first, bool last) {
      dispatch(s.fn, dim3(blocks), dim3(s.block), s.lds, stream, ev, first, last && !tail_after, a);
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (tail0 < a.S) {
    const unsigned gy = static_cast<unsigned>(std::min(a.batch, 65535));
    const uint64_t gx = (a.S - tail0 + kBlock - 1) / kBlock;
    dispatch(kByte[a.R - 1], dim3(static_cast<unsigned>(gx), gy), dim3(kBlock), 0, stream, ev,
             /*first=*/a.nvec == 0, /*last=*/true, a, tail0);
    return hipGetLastError();
  }
  return hipSuccess;
}

// ---- no-lookup ceiling (measurement only; rs_plan_launch_ceiling) ----------------------
// Policy::NOMATH turns the LDS kernel into the memory ceiling of its own traffic shape:
// the same loads, stores, grid, block size, tile order and table prologue, with the
// lookups replaced by one XOR per input dword.
// bench.py times it in the same process as the plan it bounds.
namespace {
template <int R, int ORD>
using NomathPolicy = dev::Policy<2, 1, true, true, false, 512, (R > 8 ? 4 : 2), ORD, (R > 8 ? 1 : 0), true>;
// [every order][R - 1] for R <= 8; wide groups: consecutive and Q8 (the orders they run)
// (A/B build)
const auto kNomath = ab_table<NomathPolicy, LdsPolicy, 1, 8, CALLFS_EVERY_ORDER>();
const auto kNomathWide = ab_table<NomathPolicy, LdsPolicy, 9, 8, O::kConsecutive, O::kSeg8>();

template <int... Os>
constexpr std::array<VecFn, kTileOrders> stream_read_table(std::integer_sequence<int, Os...>) {
  return {&dev::rs_stream_read<kPolicyOrd[Os]>...};
}
template <int... Os>
constexpr std::array<VecFn, kTileOrders> stream_write_table(std::integer_sequence<int, Os...>) {
  return {&dev::rs_stream_write<kPolicyOrd[Os]>...};
}
const auto kStreamRead = stream_read_table(std::make_integer_sequence<int, kTileOrders>{});
const auto kStreamWrite = stream_write_table(std::make_integer_sequence<int, kTileOrders>{});

#if CALLFS_RS_AB_INSTANCES
// modes 3..5 (probe): the write streams alone from each row's first 64 / 128 / 256-B
// boundary, consecutive tiles
const std::array<VecFn, 3> kStreamWriteAligned = {
    &dev::rs_stream_write<0, 64>, &dev::rs_stream_write<0, 128>, &dev::rs_stream_write<0, 256>};
// modes 6..8 (probe): the read streams alone from each shard's first 64 / 128 / 256-B boundary
const std::array<VecFn, 3> kStreamReadAligned = {
    &dev::rs_stream_read<0, 64>, &dev::rs_stream_read<0, 128>, &dev::rs_stream_read<0, 256>};
#endif

// The tile order the production launch of code f would take: launch_apply's resolution of the
// code (realign_order, the triple rule, the nibble rule), with three differences that are meant.
// A code's feasibility is not checked: the ceiling is measured in the order the code names.
// The double-buffered G4 / G8 triples count as G8. And the realigning and v_perm launches are
// bounded by the plain LDS kernel's traffic in the order they run in.
TileOrder ceiling_order(const ApplyArgs& a, const Traits& t, Form f) {
  const bool by_rule = f.family == Family::kRule;
  if (can_realign(a, t) && (realigning(f) || (by_rule && takes_realign(a, t)))) return realign_order(f);
  if (const auto named = named_order(f)) return *named;
  if (a.R > 8) return wide_rule(t);
  const auto tri = tri_rule_of(a, t);
  return tri ? *tri : lds_rule(a, t);
}
}  // namespace

hipError_t launch_ceiling(ApplyArgs a, hipStream_t stream, int order, int mode, LaunchEvents ev) {
  const Form f = decode_order(order);
  if (a.R < 1 || a.R > kMaxRowsPerLaunch || a.K < 1 || a.K > kMaxK || a.batch < 1 || !a.ltabs ||
      mode < 0 || mode > 8 || !f.valid())
    return hipErrorInvalidValue;
  if (!kAbInstances && mode != 1 && mode != 2) return hipErrorNotSupported;
  const Traits t(a);
  a.nvec = t.nvec;
  if (a.nvec == 0) return hipSuccess;
  const bool tail = a.nvec * 16 < a.S;
  a.tail_in_vec = tail && mode == 0 ? tail_code(a.nvec, LdsPolicy::TILE_VECS, LdsPolicy::BS) : 0u;
  const TileOrder ord = ceiling_order(a, t, f);
  const int o = static_cast<int>(ord);
  const unsigned grid = dev::vec_grid<LdsPolicy>(a.nvec, a.batch);
  VecFn fn = nullptr;
  size_t lds = 0;
  if (mode == 0) {  // the no-lookup form of the LDS kernel
    fn = a.R <= 8 ? kNomath[o][a.R - 1] : instance(kNomathWide, ord, O::kConsecutive, a.R - 9);
    lds = dev::lds_bytes(a.K, a.R);
    if (lds > (64u << 10))
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fn),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 << 10);
  } else {  // the read streams alone / the write streams alone
    fn = (mode == 1 ? kStreamRead : kStreamWrite)[o];
#if CALLFS_RS_AB_INSTANCES
    if (mode >= 3) fn = mode >= 6 ? kStreamReadAligned[mode - 6] : kStreamWriteAligned[mode - 3];
#endif
  }
  launch_sliced(grid, a, t, [&](uint32_t blocks, bool first, bool last) {
    dispatch(fn, dim3(blocks), dim3(LdsPolicy::BS), lds, stream, ev, first, last, a);
  });
  return hipGetLastError();
}

}  // namespace callfs
