// decaf377::FixedBases (include/decaf377_amd.hpp) on the GPU: a Pedersen-style two-base sum v G + r H against the
// composition of the Engine's own operations, the single-base case against GENERATOR * Fr, the RAII wrapper's moves, and
// an Engine that goes away before its FixedBases.  Built and run by tests/test_fixed_bases_gpu.py (-m gpu).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>

#include "decaf377_amd.hpp"

using namespace decaf377;

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

int main() {
  std::mt19937_64 rng(377);
  const size_t n = 1000;
  std::vector<Fr> v(n), r(n), vr(2 * n);
  for (size_t i = 0; i < n; ++i) {
    for (int b = 0; b < 32; ++b) { v[i].b[b] = (uint8_t)rng(); r[i].b[b] = (uint8_t)rng(); }
    vr[2 * i] = v[i];
    vr[2 * i + 1] = r[i];
  }
  {
    Engine e({0}, 18, true);
    // H: some other point of the group, as Elements
    std::vector<Fq> seed(1);
    seed[0].b[0] = 42;
    const Element G = Engine::generator(), H = e.encode_to_curve_element(seed)[0];
    FixedBases fb = e.fixed_bases({G, H}, 12);
    CHECK(fb && fb.size() == 2 && fb.table_bytes() > 0);
    std::vector<Element> els;
    const std::vector<Encoding> enc = fb.vartime_multiscalar_mul(vr, &els);
    CHECK(enc.size() == n && els.size() == n);
    // v G + r H by the Engine's own operations
    const std::vector<Element> vG = e.mul(std::vector<Element>(n, G), v);
    const std::vector<Element> rH = e.mul(std::vector<Element>(n, H), r);
    const std::vector<Encoding> want = e.vartime_compress(e.add(vG, rH));
    for (size_t i = 0; i < n; ++i) CHECK(enc[i] == want[i]);
    CHECK(e.vartime_compress(els) == enc);
    // one base: GENERATOR * Fr
    FixedBases g1 = e.fixed_bases({G}, 18);
    CHECK(g1.vartime_multiscalar_mul(v) == e.mul_generator(v));
    // moves keep exactly one owner
    FixedBases moved(std::move(g1));
    CHECK(!g1 && moved);
    CHECK(moved.vartime_multiscalar_mul(v) == e.mul_generator(v));
    g1 = std::move(moved);
    CHECK(g1 && !moved);
    bool threw = false;
    try { moved.vartime_multiscalar_mul(v); } catch (const std::logic_error&) { threw = true; }
    CHECK(threw);
  }
  {
    // an Engine destroyed first: its FixedBases is left empty, and its destructor does nothing
    auto* e = new Engine({0}, 18, true);
    FixedBases fb = e->fixed_bases({Engine::generator()}, 8);
    CHECK(fb);
    delete e;
    CHECK(!fb);
    bool threw = false;
    try { fb.vartime_multiscalar_mul(v); } catch (const std::logic_error&) { threw = true; }
    CHECK(threw);
  }
  std::printf("CPP_FIXED_BASES_OK\n");
  return 0;
}
