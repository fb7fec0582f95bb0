// decaf377::Engine::fixed_bases_long / FixedBases::msm_long / long_plan (include/decaf377_amd.hpp) on the GPU: Pedersen vector
// commitments over 100 generators -- more than d377_fixed_bases_create registers -- against the Engine's own multiplications
// and additions; the cut the library reports; the dense call on a long registration, msm_long on a short one, and an indexed
// sum that names base 99.  Built and run by tests/test_fixed_msm_long_gpu.py (-m gpu).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>

#include "decaf377_amd.hpp"

using namespace decaf377;

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

int main() {
  std::mt19937_64 rng(4096);
  const size_t n = 3, m = 100;
  Engine e({0}, 18, true);
  std::vector<Fq> seeds(m);
  for (size_t j = 0; j < m; ++j) seeds[j].b[0] = (uint8_t)(j + 1);
  std::vector<Element> bases = e.encode_to_curve_element(seeds);
  bases[0] = Engine::generator();
  bases[7] = Engine::identity();

  bool threw = false;
  try { e.fixed_bases(bases, 8); } catch (const DeviceError&) { threw = true; }       // the short registration stops at 64
  CHECK(threw);
  FixedBases fb = e.fixed_bases_long(bases, 8);
  CHECK(fb && fb.size() == m);

  const std::pair<size_t, size_t> cut = fb.long_plan(n);
  CHECK(cut.first >= 2 && cut.second >= 1 && cut.first * cut.second >= m && (cut.first - 1) * cut.second < m);
  CHECK(fb.long_plan(1u << 20).first == 1);                                         // more sums than lanes: one segment each

  std::vector<Fr> k(n * m);
  for (auto& s : k)
    for (int b = 0; b < 32; ++b) s.b[b] = (uint8_t)rng();
  for (int b = 0; b < 32; ++b) k[m + 3].b[b] = 0xff;                                  // 2^256 - 1: reduced mod r
  std::vector<Element> els;
  const std::vector<Encoding> enc = fb.msm_long(k, &els);
  CHECK(enc.size() == n && els.size() == n);

  std::vector<Element> tiled(n * m);
  for (size_t i = 0; i < n * m; ++i) tiled[i] = bases[i % m];
  const std::vector<Element> prod = e.mul(tiled, k);
  std::vector<Element> acc(n, Engine::identity());
  for (size_t j = 0; j < m; ++j) {
    std::vector<Element> col(n);
    for (size_t i = 0; i < n; ++i) col[i] = prod[i * m + j];
    acc = e.add(acc, col);
  }
  const std::vector<Encoding> want = e.vartime_compress(acc);
  for (size_t i = 0; i < n; ++i) CHECK(enc[i] == want[i]);
  CHECK(e.vartime_compress(els) == enc);
  CHECK(fb.vartime_multiscalar_mul(k) == enc);                                       // more than 64 bases: the same call

  // a short registration through the long call
  const std::vector<Element> five(bases.begin(), bases.begin() + 5);
  FixedBases small = e.fixed_bases(five, 12);
  const std::vector<Fr> k5(k.begin(), k.begin() + 2 * 5);
  CHECK(small.msm_long(k5) == small.vartime_multiscalar_mul(k5));

  // an indexed sum over the long registration: k G + k' B_99
  const std::vector<int> idx = {0, 99};
  const std::vector<Fr> k2 = {k[0], k[1]};
  const std::vector<Element> two = e.mul(std::vector<Element>{bases[0], bases[99]}, k2);
  CHECK(fb.msm_indexed(idx, k2, 2) == e.vartime_compress(e.add({two[0]}, {two[1]})));
  threw = false;
  try { fb.msm_indexed({0, 100}, k2, 2); } catch (const DeviceError&) { threw = true; }
  CHECK(threw);

  std::printf("CPP_FIXED_BASES_LONG_OK\n");
  return 0;
}
