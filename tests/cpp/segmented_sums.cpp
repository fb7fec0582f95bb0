// decaf377::Engine::vartime_multiscalar_mul_batch_segmented and msm_segmented_resident (include/decaf377_amd.hpp) on the GPU: sums
// of 0, 5, 1, 0, 129, 40, 9 and 0 terms in one call against the fold of the mirror's own `*` (mul) and `+` (add) and against
// vartime_multiscalar_mul_batch_ragged; the resident form on buffers of hipMalloc against the host form; empty sums and a sum of
// identities; bad offsets refused.  Built and run by tests/test_segmented_sums_gpu.py (-m gpu).
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
  const Element identity = Engine::identity();

  const std::vector<size_t> lengths = {0, 5, 1, 0, 129, 40, 9, 0};
  const size_t n = lengths.size();
  std::vector<uint64_t> off(n + 1, 0);
  for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + lengths[i];
  const size_t terms = (size_t)off[n];
  std::vector<Fq> seeds(terms);
  std::vector<Fr> k(terms);
  for (size_t i = 0; i < terms; ++i) {
    seeds[i].b[0] = (uint8_t)(i + 1); seeds[i].b[1] = (uint8_t)((i + 1) >> 8); seeds[i].b[2] = 78;
    for (int b = 0; b < 31; ++b) k[i].b[b] = (uint8_t)rng();
  }
  std::vector<Element> pts = e.encode_to_curve_element(seeds);
  for (uint64_t j = off[5]; j < off[6]; ++j) pts[j] = identity;   // the sum of 40 terms: the identity

  const std::vector<Element> prod = e.mul(pts, k);
  std::vector<Element> acc(n, identity);
  for (size_t i = 0; i < n; ++i)
    for (uint64_t j = off[i]; j < off[i + 1]; ++j) acc[i] = e.add(std::vector<Element>{acc[i]}, std::vector<Element>{prod[j]})[0];
  const std::vector<Encoding> want = e.vartime_compress(acc);

  std::vector<Encoding> encs, by_buckets;
  const std::vector<Element> sums = e.vartime_multiscalar_mul_batch_segmented(off, k, pts, &encs);
  CHECK(sums.size() == n && encs.size() == n);
  CHECK(encs == want);
  CHECK(e.vartime_compress(sums) == encs);
  for (const size_t i : {size_t(0), size_t(3), size_t(5), size_t(7)}) CHECK(encs[i] == Encoding{});
  e.vartime_multiscalar_mul_batch_ragged(off, k, pts, &by_buckets);
  CHECK(by_buckets == encs);

  DevBuf<Element> dpts(pts);
  DevBuf<Fr> dk(k);
  DevBuf<uint64_t> doff(off);
  DevBuf<Encoding> enc(n);
  DevBuf<Element> el(n);
  e.msm_segmented_resident(0, s, dpts.p, dk.p, off.data(), doff.p, n, enc.p, el.p);
  CHECK(enc.host(s) == encs);
  CHECK(e.vartime_compress(el.host(s)) == encs);
  DevBuf<Encoding> enc2(n);
  e.msm_segmented_resident(0, s, dpts.p, dk.p, off.data(), doff.p, n, enc2.p);   // without Element records
  CHECK(enc2.host(s) == encs);

  bool threw = false;
  try { e.vartime_multiscalar_mul_batch_segmented({0, 2, 1, 2}, std::vector<Fr>(2), std::vector<Element>(2, identity)); }
  catch (const DeviceError&) { threw = true; }
  CHECK(threw);
  threw = false;
  try { e.vartime_multiscalar_mul_batch_segmented({1, 2}, std::vector<Fr>(2), std::vector<Element>(2, identity)); }
  catch (const DeviceError&) { threw = true; }
  CHECK(threw);
  HIP_OK(hipStreamDestroy(s));
  std::printf("CPP_SEGMENTED_SUMS_OK\n");
  return 0;
}
