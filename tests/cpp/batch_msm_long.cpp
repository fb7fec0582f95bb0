// decaf377::Engine::vartime_multiscalar_mul_batch_long (include/decaf377_amd.hpp) on the GPU: sums of 17 and of 129 terms on
// Elements and on Encodings against the fold of the mirror's own `*` (mul) and `+` (add), an invalid Encoding left out of
// its sum, and a length the call refuses.  Built and run by tests/test_batch_msm_long_gpu.py (-m gpu).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>

#include "decaf377_amd.hpp"

using namespace decaf377;

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

int main() {
  std::mt19937_64 rng(377);
  Engine e({0}, 18, true);
  for (const size_t m : {size_t(17), size_t(129)}) {
    const size_t n = 20, terms = n * m;
    std::vector<Fq> seeds(terms);
    std::vector<Fr> k(terms);
    for (size_t i = 0; i < terms; ++i)
      for (int b = 0; b < 31; ++b) { seeds[i].b[b] = (uint8_t)rng(); k[i].b[b] = (uint8_t)rng(); }
    const std::vector<Element> pts = e.encode_to_curve_element(seeds);
    std::vector<Encoding> encs;
    const std::vector<Element> sums = e.vartime_multiscalar_mul_batch_long(m, k, pts, &encs);
    CHECK(sums.size() == n && encs.size() == n);

    // the fold: every term by `*`, then the terms of a sum one after the other by `+`, n sums side by side
    const std::vector<Element> prod = e.mul(pts, k);
    std::vector<Element> acc(n), col(n);
    for (size_t s = 0; s < n; ++s) acc[s] = prod[s * m];
    for (size_t j = 1; j < m; ++j) {
      for (size_t s = 0; s < n; ++s) col[s] = prod[s * m + j];
      acc = e.add(acc, col);
    }
    const std::vector<Encoding> want = e.vartime_compress(acc);
    for (size_t s = 0; s < n; ++s) CHECK(encs[s] == want[s]);
    CHECK(e.vartime_compress(sums) == encs);

    // on Encodings, the last term of sum 0 invalid: reported, and the sum goes without it
    std::vector<Encoding> raw = e.vartime_compress(pts);
    raw[m - 1].b[31] |= 0x40;
    std::vector<Encoding> encs2;
    const auto got = e.vartime_multiscalar_mul_batch_long_encoded(m, k, raw, &encs2);
    CHECK(got.first.size() == n && got.second.size() == terms);
    for (size_t i = 0; i < terms; ++i) CHECK(got.second[i].ok == (i != m - 1));
    for (size_t s = 1; s < n; ++s) CHECK(encs2[s] == want[s]);
    std::vector<Element> less(1, acc[0]), last(1, prod[m - 1]);
    CHECK(encs2[0] == e.vartime_compress(e.sub(less, last))[0]);
  }
  bool threw = false;
  try { e.vartime_multiscalar_mul_batch_long(5000, std::vector<Fr>(5000), std::vector<Element>(5000)); } catch (const DeviceError&) { threw = true; }
  CHECK(threw);
  std::printf("CPP_BATCH_MSM_LONG_OK\n");
  return 0;
}
