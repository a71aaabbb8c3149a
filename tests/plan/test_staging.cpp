// The layout layer of beam_slam_amd/csrc/staging.h on the CPU, for tests/test_staging.py: a stand-alone program (plain, and under
// AddressSanitizer + UndefinedBehaviorSanitizer) that walks random segment lists and the seven front-end entry points' layouts
// with a host buffer standing in for the device allocation.  Prints "OK <lists checked>" and returns 0, or names what failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "inertial_align.h"
#include "staging.h"

using bsg::StageLayout;

#define REQUIRE(cond)                                                                        \
  do { if (!(cond)) { std::printf("FAILED %s:%d list %d: %s\n", __FILE__, __LINE__, g_list, #cond); std::exit(1); } } while (0)

static int g_list = 0;
static std::mt19937 g_rng(20240607u);

enum Kind { IN, OUT, SCRATCH };
struct Spec { Kind kind; size_t bytes; bool null_ptr; };   // null_ptr: an input of no bytes without src, an output without dst

constexpr size_t kGuard = 16;
constexpr unsigned char kGuardByte = 0xA5;

// One caller array of exactly `bytes` (+ guards for an output), on the heap so that the sanitizer sees a byte past it.
struct Array {
  std::unique_ptr<unsigned char[]> mem;
  unsigned char* p = nullptr;
  std::vector<unsigned char> expect;   // input: what the caller holds; output: what the stand-in kernel wrote
};

static void check(const std::vector<Spec>& specs) {
  ++g_list;
  std::vector<Array> arr(specs.size());
  std::vector<int> id(specs.size());
  StageLayout L;
  for (size_t i = 0; i < specs.size(); ++i) {
    const Spec& s = specs[i];
    Array& a = arr[i];
    a.expect.resize(s.bytes);
    for (unsigned char& b : a.expect) b = (unsigned char)g_rng();
    if (s.kind == IN && !s.null_ptr) {
      a.mem.reset(new unsigned char[s.bytes]);
      a.p = a.mem.get();
      if (s.bytes) std::memcpy(a.p, a.expect.data(), s.bytes);
    } else if (s.kind == OUT && !s.null_ptr) {
      a.mem.reset(new unsigned char[s.bytes + 2 * kGuard]);
      std::memset(a.mem.get(), kGuardByte, s.bytes + 2 * kGuard);
      a.p = a.mem.get() + kGuard;
    }
    id[i] = s.kind == IN ? L.in(a.p, s.bytes) : s.kind == OUT ? L.out(a.p, s.bytes) : L.scratch(s.bytes);
  }
  // offsets: multiples of 256, disjoint, in declaration order; the three spans contiguous and in the order inputs, outputs, scratch
  const size_t in_end = L.in_bytes(), out_end = in_end + L.out_bytes(), total = L.total_bytes();
  REQUIRE(in_end % 256 == 0 && out_end % 256 == 0 && total % 256 == 0 && in_end <= out_end && out_end <= total);
  size_t prev_end = 0;
  int prev_kind = IN;
  for (size_t i = 0; i < specs.size(); ++i) {
    const size_t off = L.offset(id[i]), end = off + specs[i].bytes;
    REQUIRE(off % 256 == 0);
    REQUIRE(off >= prev_end && off - prev_end < 256);   // disjoint, in order, and no more apart than the alignment asks
    REQUIRE(specs[i].kind >= prev_kind);
    const size_t lo = specs[i].kind == IN ? 0 : specs[i].kind == OUT ? in_end : out_end;
    const size_t hi = specs[i].kind == IN ? in_end : specs[i].kind == OUT ? out_end : total;
    REQUIRE(off >= lo && end <= hi);
    if (specs[i].kind != prev_kind) REQUIRE(off == lo);   // a span begins with its first segment
    prev_end = end;
    prev_kind = specs[i].kind;
  }
  REQUIRE(total >= prev_end && total - prev_end < 256);
  // the round trip: pack, copy in, a kernel that fills every output segment, copy out, scatter
  std::unique_ptr<unsigned char[]> dev(new unsigned char[total]);
  std::memset(dev.get(), 0xEE, total);
  L.pack();
  if (in_end) std::memcpy(dev.get(), L.image(), in_end);
  for (size_t i = 0; i < specs.size(); ++i) {
    unsigned char* d = dev.get() + L.offset(id[i]);
    if (specs[i].kind == IN) REQUIRE(specs[i].bytes == 0 || !std::memcmp(d, arr[i].expect.data(), specs[i].bytes));
    if (specs[i].kind == OUT && specs[i].bytes) std::memcpy(d, arr[i].expect.data(), specs[i].bytes);
  }
  if (out_end > in_end) std::memcpy(L.image(), dev.get() + in_end, out_end - in_end);
  L.scatter();
  for (size_t i = 0; i < specs.size(); ++i) {
    if (specs[i].kind != OUT) continue;
    const size_t n = specs[i].bytes;
    REQUIRE(n == 0 || !std::memcmp(L.out_image<unsigned char>(id[i]), arr[i].expect.data(), n));   // through the accessor, asked for or not
    if (!arr[i].p) continue;
    REQUIRE(n == 0 || !std::memcmp(arr[i].p, arr[i].expect.data(), n));                             // through scatter()
    for (size_t g = 0; g < kGuard; ++g) REQUIRE(arr[i].p[-(std::ptrdiff_t)g - 1] == kGuardByte && arr[i].p[n + g] == kGuardByte);
  }
  // the caller's inputs are read only
  for (size_t i = 0; i < specs.size(); ++i)
    if (specs[i].kind == IN && arr[i].p) REQUIRE(specs[i].bytes == 0 || !std::memcmp(arr[i].p, arr[i].expect.data(), specs[i].bytes));
}

// ---- the seven entry points' layouts (bsgpu_frontend.cpp), n items holding m elements in all; optional outputs asked for or not
static std::vector<Spec> in_out(std::initializer_list<size_t> in, std::initializer_list<std::pair<size_t, bool>> out, std::initializer_list<size_t> scratch = {}) {
  std::vector<Spec> s;
  for (size_t b : in) s.push_back({IN, b, b == 0});
  for (const auto& o : out) s.push_back({OUT, o.first, o.second});
  for (size_t b : scratch) s.push_back({SCRATCH, b, true});
  return s;
}
constexpr size_t kCamera = 128;   // DevCamera: 16 doubles
static void real_layouts(size_t n, size_t m, bool opt_null) {
  const bool rec = true;   // a per-item record: no dst, read through the accessor
  check(in_out({4 * (n + 1), 8 * m, 24 * m, 24 * m, 8 * n, 24 * n, 24 * n, 288}, {{8 * 287 * n, false}}));                                  // preintegrate
  check(in_out({4 * (n + 1), 8 * n, 8 * m, 32 * m, 24 * m, 8 * 10 * m, 24 * 10 * m, 24 * 10 * m},                                            // inertial_alignment
               {{24 * n, false}, {24 * n, false}, {8 * n, false}, {8 * n, false}, {4 * n, false}, {4 * n, false}, {24 * m, false}, {32 * m, false},
                {24 * m, false}, {24 * m, false}},
               {4 * (m + n), 8 * m * bsg::kAlignFrameScratch, 8 * n * bsg::kAlignPathScratch}));
  check(in_out({4 * (n + 1), 8 * m, 16 * m}, {{24 * n, false}, {4 * n, false}}));                                                              // triangulate
  check(in_out({4 * (n + 1), 4 * n, 0, kCamera, 16 * m, 24 * m, 56 * n}, {{8 * 45 * n, rec}, {8 * n, rec}}));                                   // localize_frames, points
  check(in_out({4 * (n + 1), 4 * n, 4 * m, kCamera, 16 * m, 0, 56 * n}, {{8 * 45 * n, rec}, {8 * n, rec}}));                                    // localize_frames, lm_block
  check(in_out({4 * (n + 1), 32 * n, 16 * m, 16 * m}, {{72 * n, opt_null}, {32 * n, rec}, {m, false}}));                                        // essential_ransac
  check(in_out({4 * (n + 1), 4 * n, kCamera, 16 * m, 24 * m}, {{8 * 19 * n, rec}, {24 * n, rec}, {m, false}}));                                 // absolute_pose_ransac
  check(in_out({4 * (n + 1), 4 * n, kCamera, 16 * m, 16 * m}, {{8 * 27 * n, rec}, {44 * n, rec}, {24 * m, opt_null}, {m, false}, {m, opt_null}}));   // relative_pose_ransac
}

static void start_tables() {
  using namespace bsg;
  const int32_t ok[] = {0, 0, 5, 5}, off[] = {1, 2, 3, 4}, dec[] = {0, 4, 3, 9}, lng[] = {0, 2, 9, 9};
  int asked = 0;
  REQUIRE(check_start_table(ok, 3) == kStartOk && check_start_table(ok, 0) == kStartOk && check_start_table(ok, 3, 5) == kStartOk);
  REQUIRE(check_start_table(ok, 3, 4) == kStartTooLong && check_start_table(lng, 3, 6) == kStartTooLong && check_start_table(lng, 3, 7) == kStartOk);
  REQUIRE(check_start_table(off, 3) == kStartNotZero && check_start_table(off, 0) == kStartNotZero);
  REQUIRE(check_start_table(dec, 3) == kStartDecreasing && check_start_table(dec, 1) == kStartOk);
  // the order: an item is looked at after its own two offsets and before the next item's; lengths after every item
  REQUIRE(check_start_table(dec, 3, 1, [&](int k) { ++asked; return k != 0; }) == kStartBadItem && asked == 1);
  REQUIRE(check_start_table(dec, 3, 1, [&](int k) { return k != 1; }) == kStartDecreasing);
  REQUIRE(check_start_table(lng, 3, 1, [&](int k) { return k != 2; }) == kStartBadItem);
}

int main() {
  const size_t sizes[] = {0, 1, 7, 255, 256, 257, 4097};
  for (int it = 0; it < 400; ++it) {
    const int n_in = (int)(g_rng() % 6), n_out = (int)(g_rng() % 6), n_scr = (int)(g_rng() % 4);
    std::vector<Spec> specs;
    for (int i = 0; i < n_in + n_out + n_scr; ++i) {
      const Kind k = i < n_in ? IN : i < n_in + n_out ? OUT : SCRATCH;
      const size_t b = sizes[g_rng() % 7];
      // dst null with probability 1/4; src null only where there is nothing to read, then half of the time
      const bool null_ptr = k == OUT ? g_rng() % 4 == 0 : k == IN ? (b == 0 && g_rng() % 2 == 0) : true;
      specs.push_back({k, b, null_ptr});
    }
    check(specs);
  }
  for (int opt_null = 0; opt_null < 2; ++opt_null) {
    real_layouts(1, 3, opt_null != 0);    // one item
    real_layouts(3, 3, opt_null != 0);    // three items, the first and the last empty: the packed arrays are the middle one's
    real_layouts(3, 0, opt_null != 0);    // every item empty: the packed arrays have no bytes at all
  }
  start_tables();
  std::printf("OK %d\n", g_list);
  return 0;
}
