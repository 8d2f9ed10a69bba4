// Order codes: the ints that name a kernel form and its tile order across the C ABI
// (include/callfs_rs.h RS_ORDER_*, rs_plan_set_orders / rs_plan_forms, the tune-table files),
// and their one decoder. A code is a family's base plus a member of the family, in bands of
// 32; Form is what it means. Plain C++ (no HIP): tests/native/host_test.cpp round-trips every
// code.
#pragma once

#include "tile_order.hpp"

namespace callfs {

// order_candidates / launch_apply code for the realigning kernel of misaligned launches
// (tile orders are TileOrder values 0..4, which on a misaligned launch select the plain
// kernel with unaligned accesses)
// (kOrderRealign + the TileOrder it runs in: consecutive, X8 or X32)
constexpr int kOrderRealign = 32;
// (kOrderWix + a TileOrder: the R <= 4 LDS kernel with 6-bit lookups over shard triples,
// rs_apply.hpp Policy::WIX; aligned launches without Verify rows, K >= 3)
constexpr int kOrderWix = 64;
// (kOrderTri + consecutive / G2 / X32 / Q8 / Q16: the triple loop with nibble lookups)
constexpr int kOrderTri = 96;
// (kOrderRealignTri + consecutive / X8 / X32: the realigning kernel with its aligned loads
// issued in triples)
constexpr int kOrderRealignTri = 128;
// (kOrderRealign64 + consecutive / X8 / X32: misaligned inputs with 16-B-aligned outputs --
// upstream Split of an io.ReadAll body, whose parity reedsolomon allocates aligned -- in
// 64-vector waves: aligned loads realigned in registers, lane 63's neighbour vector from
// one extra single-lane load, stores unshifted in 1 KiB wave windows; rs_apply.hpp
// REALIGN 5)
constexpr int kOrderRealign64 = 160;
// (kOrderDma + consecutive / G2 / Q8 / X32: aligned R <= 8 launches with their input vectors
// staged through an LDS-DMA ring, rs_apply.hpp Policy::DMA; A/B build)
constexpr int kOrderDma = 192;
// (kOrderTriDbG + 0 / 1: R <= 4, K >= 6 double-buffered triples with the tiles of 4 / 8 stripes
// interleaved (G4 / G8); A/B build)
constexpr int kOrderTriDbG = 224;
// (kOrderBitslice + any TileOrder: the launch group's bit-sliced kernel, ApplyArgs::bs,
// DESIGN.md §5.7; every launch group gets one: the rule takes it for wide groups and
// rs_plan_tune times it for every group)
constexpr int kOrderBitslice = 256;

// The families in band order (a code below kOrderBitslice belongs to family 1 + code / 32);
// kRule = no code (-1): the tune table, else the measured rule.
enum class Family { kRule, kPlain, kRealign, kWix, kTri, kRealignTri, kRealign64, kDma, kTriDbG, kBitslice };

// What an order code means. `member` is the code's offset in its family's band when the family
// has such a member, else -1: a TileOrder for every family but kTriDbG (0 = G4, 1 = G8, on top
// of the nibble instances' G8 order). Codes without a member (between the families, or past
// kOrderBitslice + kTileOrders: the mixed and ragged plans' form codes among them) are not
// valid; launch_apply keeps serving them as it always has, each family in its fallback order.
struct Form {
  Family family = Family::kRule;
  int member = -1;
  constexpr bool valid() const { return family == Family::kRule || member >= 0; }
  constexpr bool has_order() const { return member >= 0; }
  // the tile order the form runs in (has_order() only)
  constexpr TileOrder order() const {
    return family == Family::kTriDbG ? TileOrder::kGroup8 : static_cast<TileOrder>(member);
  }
  constexpr bool operator==(const Form& o) const { return family == o.family && member == o.member; }
};

constexpr Form form_of(Family f, TileOrder o) { return Form{f, static_cast<int>(o)}; }

constexpr Form decode_order(int code) {
  if (code < 0) return Form{};
  if (code >= kOrderBitslice)
    return Form{Family::kBitslice, code - kOrderBitslice < kTileOrders ? code - kOrderBitslice : -1};
  const Family f = static_cast<Family>(1 + code / kOrderRealign);
  const int m = code % kOrderRealign;
  return Form{f, m < (f == Family::kTriDbG ? 2 : kTileOrders) ? m : -1};
}

// The code of a valid form (-1 for the rule and for a form without a member).
constexpr int encode(Form f) {
  if (f.family == Family::kRule || f.member < 0) return -1;
  return (static_cast<int>(f.family) - 1) * kOrderRealign + f.member;
}

// (kOrderDecodeCheck + consecutive: what rs_plan_forms reports for a final decode-check plan,
// DESIGN.md §5.15. A plan's form code like the mixed and ragged ones: no launch order, no
// bit-sliced form, no tune-table entry.)
constexpr int kOrderDecodeCheck = 65536;
static_assert(!decode_order(kOrderDecodeCheck).valid() && encode(decode_order(kOrderDecodeCheck)) == -1,
              "a plan form code names no launch order");

// (kOrderDecodeRepair + consecutive: rs_plan_forms of a decode-repair plan; a
// plan form code in the same way.)
constexpr int kOrderDecodeRepair = 131072;
static_assert(!decode_order(kOrderDecodeRepair).valid() && encode(decode_order(kOrderDecodeRepair)) == -1,
              "a plan form code names no launch order");

static_assert(encode(Form{Family::kRealign, 0}) == kOrderRealign && encode(Form{Family::kWix, 0}) == kOrderWix &&
                  encode(Form{Family::kTri, 0}) == kOrderTri &&
                  encode(Form{Family::kRealignTri, 0}) == kOrderRealignTri &&
                  encode(Form{Family::kRealign64, 0}) == kOrderRealign64 &&
                  encode(Form{Family::kDma, 0}) == kOrderDma && encode(Form{Family::kTriDbG, 0}) == kOrderTriDbG &&
                  encode(Form{Family::kBitslice, 0}) == kOrderBitslice,
              "the families' bands are the kOrder* constants");

}  // namespace callfs
