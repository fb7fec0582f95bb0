// decaf377::FixedBases::msm_mixed (include/decaf377_amd.hpp), two builds of one program:
//
//   plain (built and run by tests/test_msm_mixed_gpu.py, -m gpu): on the GPU, signature checks R' = s B - c A over one
//   registered basepoint and one public key per sum, and commitments with an opening v G_asset + r H + k P, against the
//   Engine's own operations; the Encoding form with an invalid Encoding, an absent term, and a bad index.
//
//   -DMSM_MIXED_HOST (built by tests/test_msm_mixed_host.py with -fsanitize=address,undefined and run as an ordinary program):
//   no GPU and no library -- the host simulation of the lane kernel (tests/host_sim/msm_mixed_sim.cpp) on a file of inputs:
//     msm_mixed_san IN OUT m bits v t n
//   IN: m base records, n x t indices, n x t fixed scalars, n x v point records, n x v variable scalars; OUT: n Encodings, then
//   n Element records.
#include <cstdio>
#include <cstdlib>

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

#if defined(MSM_MIXED_HOST)
#include "../host_sim/msm_mixed_sim.cpp"

int main(int argc, char** argv) {
  CHECK(argc == 8);
  const int m = std::atoi(argv[3]), bits = std::atoi(argv[4]), v = std::atoi(argv[5]), t = std::atoi(argv[6]);
  const size_t n = (size_t)std::atol(argv[7]);
  std::vector<uint32_t> bases((size_t)m * 32), fk(n * t * 8), pts(n * v * 32), vk(n * v * 8), enc(n * 8), el(n * 32);
  std::vector<int> idx(n * t);
  FILE* f = std::fopen(argv[1], "rb");
  CHECK(f);
  CHECK(std::fread(bases.data(), 4, bases.size(), f) == bases.size());
  CHECK(std::fread(idx.data(), 4, idx.size(), f) == idx.size());
  CHECK(std::fread(fk.data(), 4, fk.size(), f) == fk.size());
  CHECK(std::fread(pts.data(), 4, pts.size(), f) == pts.size());
  CHECK(std::fread(vk.data(), 4, vk.size(), f) == vk.size());
  std::fclose(f);
  CHECK(fx_build(bases.data(), m, bits) == 0);
  CHECK(mx_msm_mixed(idx.data(), fk.data(), t, pts.data(), vk.data(), v, n, enc.data(), el.data()) == 0);
  f = std::fopen(argv[2], "wb");
  CHECK(f);
  CHECK(std::fwrite(enc.data(), 4, enc.size(), f) == enc.size());
  CHECK(std::fwrite(el.data(), 4, el.size(), f) == el.size());
  std::fclose(f);
  std::printf("MSM_MIXED_HOST_OK\n");
  return 0;
}

#else
#include <random>
#include <utility>

#include "decaf377_amd.hpp"

using namespace decaf377;

int main() {
  std::mt19937_64 rng(377);
  const size_t n = 1000, assets = 6, m = assets + 1;           // base m - 1 is the blinding generator H
  Engine e({0}, 18, true);
  std::vector<Fq> seeds(m + n);
  for (size_t j = 0; j < m + n; ++j) { seeds[j].b[0] = (uint8_t)(j + 1); seeds[j].b[1] = (uint8_t)((j + 1) >> 8); }
  const std::vector<Element> all = e.encode_to_curve_element(seeds);
  std::vector<Element> bases(all.begin(), all.begin() + m), A(all.begin() + m, all.end());   // A: one public key per sum
  bases[0] = Engine::generator();
  FixedBases fb = e.fixed_bases(bases, 12);
  CHECK(fb && fb.size() == m);
  auto random_fr = [&](std::vector<Fr>& k) { for (auto& x : k) for (int b = 0; b < 32; ++b) x.b[b] = (uint8_t)rng(); };

  // the signature check s B - c A (the caller negates c): t = v = 1 on base 0
  std::vector<Fr> s(n), c(n);
  random_fr(s); random_fr(c);
  const std::vector<int> zero(n, 0);
  std::vector<Element> els;
  const std::vector<Encoding> sig = fb.msm_mixed(zero, s, 1, A, c, 1, &els);
  CHECK(sig.size() == n && els.size() == n);
  const std::vector<Element> sB = e.mul(std::vector<Element>(n, bases[0]), s), cA = e.mul(A, c);
  CHECK(sig == e.vartime_compress(e.add(sB, cA)));
  CHECK(e.vartime_compress(els) == sig);

  // the commitment with an opening: v G_asset + r H + k P
  std::vector<Fr> vr(2 * n), k(n);
  random_fr(vr); random_fr(k);
  std::vector<int> idx(2 * n);
  std::vector<Element> Ga(n);
  std::vector<Fr> vv(n), rr(n);
  for (size_t i = 0; i < n; ++i) {
    const int a = (int)(rng() % assets);
    idx[2 * i] = a;
    idx[2 * i + 1] = (int)m - 1;
    Ga[i] = bases[a];
    vv[i] = vr[2 * i];
    rr[i] = vr[2 * i + 1];
  }
  const std::vector<Element> vG = e.mul(Ga, vv), rH = e.mul(std::vector<Element>(n, bases[m - 1]), rr), kP = e.mul(A, k);
  const std::vector<Encoding> want = e.vartime_compress(e.add(e.add(vG, rH), kP));
  CHECK(fb.msm_mixed(idx, vr, 2, A, k, 1) == want);

  // the blinding term absent: v G_asset + k P
  std::vector<int> absent(idx);
  for (size_t i = 0; i < n; ++i) absent[2 * i + 1] = -1;
  CHECK(fb.msm_mixed(absent, vr, 2, A, k, 1) == e.vartime_compress(e.add(vG, kP)));

  // the points as Encodings, one of them invalid: status names it and only that term is dropped
  std::vector<Encoding> Aenc = e.vartime_compress(A);
  for (int b = 0; b < 32; ++b) Aenc[7].b[b] = 0xFF;
  std::vector<uint8_t> status;
  const std::vector<Encoding> got = fb.msm_mixed(idx, vr, 2, Aenc, k, 1, &status);
  CHECK(status.size() == n);
  const std::vector<Encoding> vGrH = e.vartime_compress(e.add(vG, rH));
  for (size_t i = 0; i < n; ++i) {
    CHECK(status[i] == (i == 7 ? 1 : 0));
    CHECK(got[i] == (i == 7 ? vGrH[i] : want[i]));
  }

  // an index that names no base: refused, by the library; lengths that do not match: by the wrapper
  bool threw = false;
  std::vector<int> bad(idx);
  bad[5] = (int)m;
  try { fb.msm_mixed(bad, vr, 2, A, k, 1); } catch (const DeviceError&) { threw = true; }
  CHECK(threw);
  threw = false;
  try { fb.msm_mixed(idx, vr, 3, A, k, 1); } catch (const std::invalid_argument&) { threw = true; }
  CHECK(threw);

  std::printf("CPP_MSM_MIXED_OK\n");
  return 0;
}
#endif
