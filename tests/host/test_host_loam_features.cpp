// bs_models::scan_registration::LoamFeatureExtractor (beam_slam_amd/host/loam_feature_extractor.h): ExtractFeatures and the batched
// ExtractAll around bsgpu_extract_loam_features.  Built three ways by tests/test_host_loam_features.py:
//   -DLOAM_NO_DEVICE     the shared header on one core only (device < 0): the batch against its lone calls;
//   -DLOAM_NO_BACKEND    nothing defines the entry point: a device extractor extracts nothing (the header path still works);
//   with libbsgpu.so     the same clouds three ways — header, device one by one, device batched.
// Every way prints its clouds as ROW lines, which the Python side compares as text (%.17g: bit for bit); the weak surfaces, most of a
// scan, as their number and a sum of their bits.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../beam_slam_amd/host/loam_feature_extractor.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using namespace bs_models::scan_registration;

static void row(const char* way, int k, const LoamFeatureCloud& c) {
  std::printf("ROW %s %d %d %zu %zu %zu %zu", way, k, c.ok ? 1 : 0, c.edges.size() / 3, c.surfaces.size() / 3, c.weak_edges.size() / 3, c.weak_surfaces.size() / 3);
  for (const std::vector<double>* v : {&c.edges, &c.surfaces, &c.weak_edges}) for (double x : *v) std::printf(" %.17g", x);
  unsigned long long sum = 0;
  for (size_t i = 0; i < c.weak_surfaces.size(); ++i) {
    unsigned long long bits;
    std::memcpy(&bits, &c.weak_surfaces[i], 8);
    sum = sum * 1099511628211ull + bits;
  }
  std::printf(" %016llx\n", sum);
}

int main() {
  // a box room seen from inside: 16 beams over 30 degrees, a sweep of 100 degrees in 400 steps, 1 cm noise along the ray, in firing order
  uint64_t lcg = 2025;
  const auto uni = [&] { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (double)(lcg >> 11) / 9007199254740992.0 - 0.5; };
  const double box[3] = {20.0, 14.0, 5.0};
  const auto sweep = [&](double ox, double oy, double oz, double first_deg, int azimuths, std::vector<int32_t>* ring) {
    std::vector<double> c;
    const double rad = 3.14159265358979323846 / 180.0, o[3] = {ox, oy, oz};
    for (int a = 0; a < azimuths; ++a)
      for (int r = 0; r < 16; ++r) {
        const double el = (-15.0 + 2.0 * r) * rad, az = (first_deg + 0.25 * a) * rad;
        const double d[3] = {std::cos(el) * std::cos(az), std::cos(el) * std::sin(az), std::sin(el)};
        double t = 1e9;
        for (int k = 0; k < 3; ++k) if (d[k] != 0.0) t = std::fmin(t, ((d[k] > 0.0 ? 0.5 : -0.5) * box[k] - o[k]) / d[k]);
        t += 0.04 * uni() * 0.5;
        for (int k = 0; k < 3; ++k) c.push_back(d[k] * t);
        ring->push_back(r);
      }
    return c;
  };
  std::vector<int32_t> ring[3];
  const std::vector<double> scans[3] = {sweep(1.5, -0.8, 0.3, 10.0, 400, &ring[0]), sweep(-2.0, 1.0, -0.4, 200.0, 250, &ring[1]), {}};
  const std::vector<const std::vector<double>*> sp = {&scans[0], &scans[1], &scans[2]};
  const std::vector<const std::vector<int32_t>*> rp = {&ring[0], &ring[1], &ring[2]};

  const auto run = [&](const char* way, int device, bool batched, bool with_ring) {
    LoamFeatureExtractor x(device);
    std::vector<LoamFeatureCloud> out;
    if (batched) out = x.ExtractAll(sp, with_ring ? rp : std::vector<const std::vector<int32_t>*>{});
    else for (int k = 0; k < 3; ++k) out.push_back(x.ExtractFeatures(scans[k], with_ring ? &ring[k] : nullptr));
    for (int k = 0; k < 3; ++k) row(way, k, out[(size_t)k]);
    return out;
  };
  const std::vector<LoamFeatureCloud> header = run("HEADER", -1, true, false);
  run("HEADER_LONE", -1, false, false);
  run("HEADER_RING", -1, true, true);
  for (int k = 0; k < 2; ++k) {
    CHECK(header[k].ok && header[k].edges.size() / 3 > 10 && header[k].surfaces.size() / 3 > 100);
    CHECK((header[k].edges.size() + header[k].surfaces.size() + header[k].weak_edges.size() + header[k].weak_surfaces.size()) <= scans[k].size());
  }
  CHECK(header[2].ok && header[2].edges.empty() && header[2].surfaces.empty() && header[2].weak_surfaces.empty());
#if defined(LOAM_NO_BACKEND)
  const std::vector<LoamFeatureCloud> none = run("NONE", 0, true, false);
  for (int k = 0; k < 3; ++k) CHECK(!none[k].ok && none[k].edges.empty());
#elif !defined(LOAM_NO_DEVICE)
  CHECK(bsgpu_abi_version() == 1);      // a strong reference: the header's is weak
  run("DEVICE", 0, true, false);
  run("DEVICE_LONE", 0, false, false);
  run("DEVICE_RING", 0, true, true);
#endif
  if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
  std::printf("HOST LOAM FEATURE EXTRACTOR DONE\n");
  return 0;
}
