// The chunk pipeline of the host-memory batch routes on the CPU: rs_host.cpp,
// rs_plan.cpp, rs_context.cpp and the kernel files compiled for the host only and linked against
// the HIP stand-ins (fake_hip_runtime.cpp, fake_hip_memory.cpp: device memory is host memory, a
// copy is a memcpy, a kernel is recorded and does nothing). tests/test_native_host_routes.py
// runs it with a 64 KiB chunk budget, so that every call below runs through more chunks than a
// lane has slots: stripes cut into column parts, S % 16 != 0, a stripe shorter than a vector.
// Per call the program checks
//   - the return code and every stripe's status (RS_OK: nothing compares unequal, since the
//     status words and counts come back as the zeros that went in),
//   - the 16 guard bytes on each side of every caller buffer, and every byte of a buffer the
//     call may only read,
//   - for the update calls every parity byte: the D2H returns what the H2D sent, so a row that
//     comes back unchanged was copied out to the address and column it was staged from, across
//     column parts and slot reuse,
// and prints the deltas of rs_host_counters, the uploads, the async copies by direction and the
// recorded dispatches, which the test compares with recorded values. Every call runs twice: the
// second run finds its tables on the lane.
// With the argument "inplace" (and CALLFS_RS_INPLACE_PIPELINE=1 in the environment) the encode
// and reconstruct calls alone, on the in-place transport.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/callfs_rs.h"
#include "fake_hip_memory.hpp"
#include "fake_hip_runtime.hpp"

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

namespace {

constexpr int K = 4, M = 2, N = K + M;
constexpr size_t kGuard = 16;
constexpr uint8_t kGuardByte = 0xC3;
const std::vector<size_t> kSizes = {100003, 17, 8197, 40003, 9, 65536};
constexpr int kSlots = 3;  // a lane's default pipeline depth

// Caller buffers with guard bytes on each side; `before` is what add() filled in.
struct Arena {
  struct Buf {
    std::vector<uint8_t> bytes, before;
  };
  std::vector<std::unique_ptr<Buf>> bufs;
  uint32_t seed = 1;
  uint8_t* add(size_t n) {
    bufs.emplace_back(new Buf);
    Buf& b = *bufs.back();
    b.bytes.assign(n + 2 * kGuard, kGuardByte);
    for (size_t i = 0; i < n; ++i) {
      seed = seed * 1664525u + 1013904223u;
      b.bytes[kGuard + i] = static_cast<uint8_t>(seed >> 24);
    }
    b.before = b.bytes;
    return b.bytes.data() + kGuard;
  }
  const Buf& of(const uint8_t* p) const {
    for (const auto& b : bufs)
      if (b->bytes.data() + kGuard == p) return *b;
    CHECK(!"a buffer of this arena");
    return *bufs[0];
  }
  bool unchanged(const uint8_t* p) const { return of(p).bytes == of(p).before; }
  bool guards_intact() const {
    for (const auto& b : bufs)
      for (size_t i = 0; i < kGuard; ++i)
        if (b->bytes[i] != kGuardByte || b->bytes[b->bytes.size() - 1 - i] != kGuardByte) return false;
    return true;
  }
};

struct Probe {
  rs_host_counters c;
  size_t uploads;
  fake_mem::AsyncCopies async;
};
Probe probe(rs_ctx* ctx) {
  Probe p{};
  CHECK(rs_host_counters_read(ctx, &p.c) == RS_OK);
  p.uploads = fake_mem::uploads().size();
  p.async = fake_mem::async_copies();
  return p;
}

// One line of deltas, then the dispatched kernels with how often each ran.
void report(rs_ctx* ctx, const std::string& name, const Probe& a) {
  const Probe b = probe(ctx);
  std::vector<std::string> order;
  std::map<std::string, long> times;
  long dispatches = 0;
  unsigned long long blocks = 0;
  size_t at = 0;
  while (at < fake::log.size()) {
    const size_t end = std::min(fake::log.find('\n', at), fake::log.size());
    const std::string line = fake::log.substr(at, end - at);
    at = end + 1;
    if (line.rfind("  attr ", 0) == 0 || line.rfind("  ", 0) != 0) continue;
    const size_t sp = line.find(' ', 2);
    const std::string sym = line.substr(2, sp - 2);
    unsigned gx = 0, gy = 0;
    CHECK(std::sscanf(line.c_str() + sp, " grid=%u,%u", &gx, &gy) == 2);
    if (!times.count(sym)) order.push_back(sym);
    ++times[sym];
    ++dispatches;
    blocks += static_cast<unsigned long long>(gx) * gy;
  }
  const unsigned long long chunks = b.c.chunks - a.c.chunks;
  std::printf("case %s: calls=%llu chunks=%llu launches=%llu copies=%llu uploads=%zu h2d=%ld d2h=%ld "
              "dispatches=%ld blocks=%llu\n",
              name.c_str(), static_cast<unsigned long long>(b.c.calls - a.c.calls), chunks,
              static_cast<unsigned long long>(b.c.launches - a.c.launches),
              static_cast<unsigned long long>(b.c.copies - a.c.copies), b.uploads - a.uploads,
              b.async.h2d - a.async.h2d, b.async.d2h - a.async.d2h, dispatches, blocks);
  for (const std::string& s : order) std::printf("dispatch %s x%ld\n", s.c_str(), times[s]);
  CHECK(chunks > static_cast<unsigned long long>(kSlots));
}

// Runs `call` twice on fresh buffers: "<name>" and "<name>.again".
template <class F>
void twice(rs_ctx* ctx, const char* name, F call) {
  for (int pass = 0; pass < 2; ++pass) {
    fake::log.clear();
    const Probe before = probe(ctx);
    call();
    report(ctx, std::string(name) + (pass ? ".again" : ""), before);
  }
}

const int B = static_cast<int>(kSizes.size());

void all_ok(const std::vector<int>& status) {
  for (int s : status) CHECK(s == RS_OK);
}

void encode(rs_ctx* ctx) {
  Arena A;
  std::vector<const uint8_t*> data;
  std::vector<uint8_t*> parity;
  for (int b = 0; b < B; ++b) {
    for (int i = 0; i < K; ++i) data.push_back(A.add(kSizes[b]));
    for (int j = 0; j < M; ++j) parity.push_back(A.add(kSizes[b]));
  }
  std::vector<int> status(B, -99);
  CHECK(rs_encode_batch(ctx, K, M, B, kSizes.data(), data.data(), parity.data(), status.data()) == RS_OK);
  all_ok(status);
  CHECK(A.guards_intact());
  for (const uint8_t* p : data) CHECK(A.unchanged(p));
}

// lost[b]: the shards stripe b has lost (lens 0); required (nullable) as the call takes it.
// A lost shard that is not wanted keeps its bytes.
void reconstruct(rs_ctx* ctx, const std::vector<std::vector<int>>& lost, const std::vector<std::vector<int>>* wanted,
                 int verify) {
  Arena A;
  std::vector<uint8_t*> shards;
  std::vector<size_t> lens;
  std::vector<uint8_t> required(static_cast<size_t>(B) * N, 0), written(static_cast<size_t>(B) * N, 0);
  for (int b = 0; b < B; ++b) {
    for (int i = 0; i < N; ++i) {
      shards.push_back(A.add(kSizes[b]));
      lens.push_back(kSizes[b]);
    }
    for (int i : lost[b]) {
      lens[static_cast<size_t>(b) * N + i] = 0;
      written[static_cast<size_t>(b) * N + i] = wanted == nullptr;
    }
    if (wanted)
      for (int i : (*wanted)[b]) required[static_cast<size_t>(b) * N + i] = written[static_cast<size_t>(b) * N + i] = 1;
  }
  const std::vector<size_t> lens0 = lens;
  std::vector<int> status(B, -99);
  const int rc = wanted ? rs_reconstruct_some_batch(ctx, K, M, B, shards.data(), lens.data(), required.data(),
                                                    verify, status.data())
                        : rs_reconstruct_batch(ctx, K, M, B, shards.data(), lens.data(), verify, status.data());
  CHECK(rc == RS_OK);
  all_ok(status);
  CHECK(A.guards_intact());
  for (size_t q = 0; q < shards.size(); ++q) {
    if (!written[q]) CHECK(A.unchanged(shards[q]));
    CHECK(lens[q] == (written[q] ? kSizes[q / N] : lens0[q]));
  }
}

// pair: rs_update_batch with one or two changed shards per stripe; else rs_encode_idx on the
// largest size alone.
void update(rs_ctx* ctx, bool pair) {
  Arena A;
  if (!pair) {
    const uint8_t* shard = A.add(kSizes[0]);
    std::vector<uint8_t*> parity;
    for (int j = 0; j < M; ++j) parity.push_back(A.add(kSizes[0]));
    CHECK(rs_encode_idx(ctx, K, M, kSizes[0], shard, 2, parity.data()) == RS_OK);
    CHECK(A.guards_intact());
    for (const auto& b : A.bufs) CHECK(b->bytes == b->before);
    return;
  }
  std::vector<const uint8_t*> old_data(static_cast<size_t>(B) * K, nullptr), new_data(old_data);
  std::vector<uint8_t*> parity;
  for (int b = 0; b < B; ++b) {
    for (int i = 0; i < K; ++i) {
      if (i != b % K && !(b % 3 == 0 && i == 3)) continue;  // two changed-shard patterns and more
      old_data[static_cast<size_t>(b) * K + i] = A.add(kSizes[b]);
      new_data[static_cast<size_t>(b) * K + i] = A.add(kSizes[b]);
    }
    for (int j = 0; j < M; ++j) parity.push_back(A.add(kSizes[b]));
  }
  std::vector<int> status(B, -99);
  CHECK(rs_update_batch(ctx, K, M, B, kSizes.data(), old_data.data(), new_data.data(), parity.data(),
                        status.data()) == RS_OK);
  all_ok(status);
  CHECK(A.guards_intact());
  for (const auto& b : A.bufs) CHECK(b->bytes == b->before);  // sources, and parity byte for byte
}

// kind 0: rs_locate_batch, 1: rs_locate_batch_ex with max_errors 2, 2: rs_correct_batch.
void locate(rs_ctx* ctx, int kind) {
  Arena A;
  std::vector<uint8_t*> shards;
  std::vector<size_t> lens;
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < N; ++i) {
      shards.push_back(A.add(kSizes[b]));
      lens.push_back(kSizes[b]);
    }
  lens[static_cast<size_t>(1) * N + 5] = 0;  // a second pattern: one compared row
  std::vector<uint64_t> counts(static_cast<size_t>(B) * (N + 1), 77);
  std::vector<int> status(B, -99);
  const uint8_t* const* cs = shards.data();
  const int rc = kind == 0   ? rs_locate_batch(ctx, K, M, B, cs, lens.data(), counts.data(), status.data())
                 : kind == 1 ? rs_locate_batch_ex(ctx, K, M, B, cs, lens.data(), counts.data(), status.data(), 2)
                             : rs_correct_batch(ctx, K, M, B, shards.data(), lens.data(), counts.data(), status.data());
  CHECK(rc == RS_OK);
  all_ok(status);
  for (uint64_t c : counts) CHECK(c == 0);
  CHECK(A.guards_intact());
  for (const auto& b : A.bufs) CHECK(b->bytes == b->before);
}

}  // namespace

int main(int argc, char** argv) {
  const bool inplace = argc > 1 && std::string(argv[1]) == "inplace";
  fake::device = 0;
  fake::bs_mode = 0;
  rs_ctx* ctx = nullptr;
  CHECK(rs_init(&ctx, 0) == RS_OK);
  // one lost shard per stripe, two patterns (a data shard, a parity shard), the rest compared
  std::vector<std::vector<int>> lost1, lost2, want2;
  for (int b = 0; b < B; ++b) {
    lost1.push_back({b % 2 ? 4 : 1});
    lost2.push_back(b % 2 ? std::vector<int>{2, 3} : std::vector<int>{0, 5});
    want2.push_back({b % 2 ? 3 : 0});
  }
  twice(ctx, "encode", [&] { encode(ctx); });
  twice(ctx, "reconstruct", [&] { reconstruct(ctx, lost1, nullptr, 1); });
  if (!inplace) {
    twice(ctx, "reconstruct-some", [&] { reconstruct(ctx, lost2, &want2, 0); });
    twice(ctx, "update-pair", [&] { update(ctx, true); });
    twice(ctx, "encode-idx", [&] { update(ctx, false); });
    twice(ctx, "locate", [&] { locate(ctx, 0); });
    twice(ctx, "locate2", [&] { locate(ctx, 1); });
    twice(ctx, "correct", [&] { locate(ctx, 2); });
  }
  rs_shutdown(ctx);
  std::printf("host_routes ok\n");
  return 0;
}
