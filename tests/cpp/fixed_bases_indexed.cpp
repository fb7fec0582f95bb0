// decaf377::FixedBases::msm_indexed (include/decaf377_amd.hpp) on the GPU: value commitments v G_asset + r H over a
// registration of several asset generators plus the blinding generator, each sum naming its two bases, against the Engine's
// own operations; an absent term, a repeated base, the index row 0 .. m-1 against the dense call, and a bad index.
// Built and run by tests/test_fixed_bases_indexed_gpu.py (-m gpu).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>

#include "decaf377_amd.hpp"

using namespace decaf377;

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

int main() {
  std::mt19937_64 rng(377);
  const size_t n = 1000, assets = 6, m = assets + 1;           // base m - 1 is the blinding generator H
  Engine e({0}, 18, true);
  std::vector<Fq> seeds(m);
  for (size_t j = 0; j < m; ++j) seeds[j].b[0] = (uint8_t)(j + 1);
  std::vector<Element> bases = e.encode_to_curve_element(seeds);
  bases[0] = Engine::generator();
  FixedBases fb = e.fixed_bases(bases, 12);
  CHECK(fb && fb.size() == m);

  std::vector<Fr> v(n), r(n), vr(2 * n);
  std::vector<int> idx(2 * n);
  std::vector<Element> Ga(n);
  for (size_t i = 0; i < n; ++i) {
    for (int b = 0; b < 32; ++b) { v[i].b[b] = (uint8_t)rng(); r[i].b[b] = (uint8_t)rng(); }
    const int a = (int)(rng() % assets);
    idx[2 * i] = a;
    idx[2 * i + 1] = (int)m - 1;
    vr[2 * i] = v[i];
    vr[2 * i + 1] = r[i];
    Ga[i] = bases[a];
  }
  std::vector<Element> els;
  const std::vector<Encoding> enc = fb.msm_indexed(idx, vr, 2, &els);
  CHECK(enc.size() == n && els.size() == n);
  const std::vector<Element> vG = e.mul(Ga, v);
  const std::vector<Element> rH = e.mul(std::vector<Element>(n, bases[m - 1]), r);
  const std::vector<Encoding> want = e.vartime_compress(e.add(vG, rH));
  for (size_t i = 0; i < n; ++i) CHECK(enc[i] == want[i]);
  CHECK(e.vartime_compress(els) == enc);

  // the blinding term absent: v G_asset alone; the asset twice: (v + v) G_asset
  std::vector<int> absent(idx), twice(idx);
  std::vector<Fr> vv(vr);
  for (size_t i = 0; i < n; ++i) { absent[2 * i + 1] = -1; twice[2 * i + 1] = twice[2 * i]; vv[2 * i + 1] = v[i]; }
  CHECK(fb.msm_indexed(absent, vr, 2) == e.vartime_compress(vG));
  CHECK(fb.msm_indexed(twice, vv, 2) == e.vartime_compress(e.add(vG, vG)));

  // every base in registration order: the dense call
  const size_t nd = 100;
  std::vector<Fr> kd(nd * m);
  std::vector<int> all(nd * m);
  for (size_t i = 0; i < nd * m; ++i) {
    for (int b = 0; b < 32; ++b) kd[i].b[b] = (uint8_t)rng();
    all[i] = (int)(i % m);
  }
  CHECK(fb.msm_indexed(all, kd, m) == fb.vartime_multiscalar_mul(kd));

  // an index that names no base: refused, by the library
  bool threw = false;
  std::vector<int> bad(idx);
  bad[5] = (int)m;
  try { fb.msm_indexed(bad, vr, 2); } catch (const DeviceError&) { threw = true; }
  CHECK(threw);
  threw = false;
  try { fb.msm_indexed(idx, vr, 3); } catch (const std::invalid_argument&) { threw = true; }
  CHECK(threw);

  std::printf("CPP_FIXED_BASES_INDEXED_OK\n");
  return 0;
}
