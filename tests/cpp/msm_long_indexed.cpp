// decaf377::Engine::vartime_multiscalar_mul_batch_long_indexed, msm_long_indexed_resident and msm_long_resident
// (include/decaf377_amd.hpp) on the GPU: sums of 5, 17 and 129 terms over a pool of 23 points, with absent terms, against the
// fold of the mirror's own `*` (mul) and `+` (add) on the gathered points; the resident forms on buffers of hipMalloc against
// the host forms; a planted index in the verdict, and one the host form refuses.  Built and run by
// tests/test_msm_long_resident_gpu.py (-m gpu).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "decaf377_amd.hpp"

using namespace decaf377;

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)
#define HIP_OK(e) CHECK((e) == hipSuccess)

template <class T>
struct DevBuf {                                                // a hipMalloc'ed copy of a host vector
  T* p = nullptr;
  size_t n;
  explicit DevBuf(size_t count) : n(count) { HIP_OK(hipMalloc(reinterpret_cast<void**>(&p), (count ? count : 1) * sizeof(T))); }
  explicit DevBuf(const std::vector<T>& h) : DevBuf(h.size()) { HIP_OK(hipMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice)); }
  ~DevBuf() { (void)hipFree(p); }
  std::vector<T> host(hipStream_t s) const {
    std::vector<T> h(n);
    HIP_OK(hipStreamSynchronize(s));
    HIP_OK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
    return h;
  }
};

int main() {
  std::mt19937_64 rng(377);
  Engine e({0}, 18, true);
  HIP_OK(hipSetDevice(0));
  hipStream_t s;
  HIP_OK(hipStreamCreate(&s));
  const size_t count = 23;
  std::vector<Fq> seeds(count);
  for (size_t j = 0; j < count; ++j) seeds[j].b[0] = (uint8_t)(j + 1);
  const std::vector<Element> pool = e.encode_to_curve_element(seeds);
  const Element identity = Engine::identity();
  DevBuf<Element> dpool(pool);

  for (const size_t m : {size_t(5), size_t(17), size_t(129)}) {
    const size_t n = 6, terms = n * m;
    std::vector<Fr> k(terms);
    std::vector<int> idx(terms);
    for (size_t i = 0; i < terms; ++i) {
      for (int b = 0; b < 31; ++b) k[i].b[b] = (uint8_t)rng();
      idx[i] = (i % 7 == 3) ? -1 : (int)(rng() % count);
    }
    idx[0] = 0; idx[1] = (int)count - 1;
    for (size_t j = 0; j < m; ++j) idx[(n - 1) * m + j] = -1;  // the last sum: every term absent
    std::vector<Encoding> encs;
    const std::vector<Element> sums = e.vartime_multiscalar_mul_batch_long_indexed(m, pool, idx, k, &encs);
    CHECK(sums.size() == n && encs.size() == n);

    // the fold: every term's gathered point by `*` (an absent term the identity), then the terms of a sum by `+`
    std::vector<Element> pts(terms);
    for (size_t i = 0; i < terms; ++i) pts[i] = idx[i] < 0 ? identity : pool[(size_t)idx[i]];
    const std::vector<Element> prod = e.mul(pts, k);
    std::vector<Element> acc(n), col(n);
    for (size_t i = 0; i < n; ++i) acc[i] = prod[i * m];
    for (size_t j = 1; j < m; ++j) {
      for (size_t i = 0; i < n; ++i) col[i] = prod[i * m + j];
      acc = e.add(acc, col);
    }
    const std::vector<Encoding> want = e.vartime_compress(acc);
    CHECK(encs == want);
    CHECK(e.vartime_compress(sums) == encs);
    CHECK(encs[n - 1] == Encoding{});                           // all absent: the all-zero Encoding

    // the resident forms against the host forms
    DevBuf<int> di(idx);
    DevBuf<Fr> dk(k);
    DevBuf<Encoding> enc(n);
    DevBuf<Element> el(n);
    DevBuf<uint64_t> verdict(2);
    e.msm_long_indexed_resident(0, s, dpool.p, count, di.p, dk.p, m, n, enc.p, el.p, verdict.p);
    CHECK(enc.host(s) == encs);
    CHECK(e.vartime_compress(el.host(s)) == encs);
    CHECK(verdict.host(s) == (std::vector<uint64_t>{0, UINT64_MAX}));
    DevBuf<Element> dpts(pts);
    e.msm_long_resident(0, s, dpts.p, dk.p, m, n, enc.p, el.p);
    CHECK(enc.host(s) == encs);

    // an index outside the pool: counted and walked as absent by the resident form, refused by the host form
    std::vector<int> bad(idx), mended(idx);
    bad[2] = (int)count; bad[m + 1] = -2;
    mended[2] = mended[m + 1] = -1;
    DevBuf<int> dbad(bad);
    e.msm_long_indexed_resident(0, s, dpool.p, count, dbad.p, dk.p, m, n, enc.p, nullptr, verdict.p);
    std::vector<Encoding> mended_enc;
    e.vartime_multiscalar_mul_batch_long_indexed(m, pool, mended, k, &mended_enc);
    CHECK(enc.host(s) == mended_enc);
    CHECK(verdict.host(s) == (std::vector<uint64_t>{2, 2}));
    bool threw = false;
    try { e.vartime_multiscalar_mul_batch_long_indexed(m, pool, bad, k); } catch (const DeviceError&) { threw = true; }
    CHECK(threw);
  }
  HIP_OK(hipStreamDestroy(s));
  std::printf("CPP_MSM_LONG_INDEXED_OK\n");
  return 0;
}
