// The resident forms of the sums over registered bases (include/decaf377_amd.hpp: FixedBases::msm_resident, msm_long_resident,
// msm_indexed_resident, msm_mixed_resident, check_base_index_resident), two builds of one program:
//
//   plain (built and run by tests/test_resident_sums_gpu.py, -m gpu): on the GPU, every resident wrapper on buffers of
//   hipMalloc against its host form on the same inputs, on a stream of the program's own; a planted index in the verdict.
//
//   -DINDEX_VERDICT_HOST (built by tests/test_resident_sums_host.py, also with -fsanitize=address,undefined, and run as an
//   ordinary program): no GPU and no library -- index_verdict.hpp alone, folded as k_index_verdict folds it: lanes that stride
//   over the array, the lanes of a wave of 64 joined, then the waves.
//     index_verdict_host m lanes < ints        prints "count first" (first = 18446744073709551615 where there is none)
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

#if defined(INDEX_VERDICT_HOST)
#include "index_verdict.hpp"

using namespace d377;

int main(int argc, char** argv) {
  CHECK(argc == 3);
  const int m = std::atoi(argv[1]);
  const size_t lanes = (size_t)std::atol(argv[2]);            // the pretended grid: a multiple of 64
  CHECK(lanes > 0 && lanes % 64 == 0);
  std::vector<int> idx;
  for (long long x; std::scanf("%lld", &x) == 1;) idx.push_back((int)x);
  std::vector<IndexVerdict> lane(lanes, verdict_none());
  for (size_t l = 0; l < lanes; ++l)
    for (size_t p = l; p < idx.size(); p += lanes) lane[l] = verdict_join(lane[l], verdict_of(idx[p], m, (uint64_t)p));
  IndexVerdict record = verdict_none();
  for (size_t w = 0; w < lanes / 64; ++w) {
    IndexVerdict wave[64];
    for (int l = 0; l < 64; ++l) wave[l] = lane[w * 64 + l];
    for (int off = 32; off > 0; off >>= 1)                     // the butterfly: every lane ends with the wave's verdict
      for (int l = 0; l < 64; ++l)
        if ((l & off) == 0) wave[l] = wave[l ^ off] = verdict_join(wave[l], wave[l ^ off]);
    if (wave[0].count != 0) record = verdict_join(record, wave[0]);
  }
  std::printf("%llu %llu\n", (unsigned long long)record.count, (unsigned long long)record.first);
  return 0;
}

#else
#include <cstring>
#include <random>

#include <hip/hip_runtime_api.h>

#include "decaf377_amd.hpp"

using namespace decaf377;

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
  const size_t n = 257, m = 5, t = 2, v = 1;
  Engine e({0}, 18, true);
  HIP_OK(hipSetDevice(0));
  hipStream_t s;
  HIP_OK(hipStreamCreate(&s));
  std::vector<Fq> seeds(m + n);
  for (size_t j = 0; j < m + n; ++j) { seeds[j].b[0] = (uint8_t)(j + 1); seeds[j].b[1] = (uint8_t)((j + 1) >> 8); }
  const std::vector<Element> all = e.encode_to_curve_element(seeds);
  const std::vector<Element> bases(all.begin(), all.begin() + m), A(all.begin() + m, all.end());
  FixedBases fb = e.fixed_bases(bases, 8);
  auto random_fr = [&](std::vector<Fr>& k) { for (auto& x : k) for (int b = 0; b < 32; ++b) x.b[b] = (uint8_t)rng(); };

  // the dense sums, one lane per sum and cut into segments
  std::vector<Fr> dk(n * m);
  random_fr(dk);
  {
    DevBuf<Fr> k(dk);
    DevBuf<Encoding> enc(n);
    DevBuf<Element> el(n);
    fb.msm_resident(0, s, k.p, n, enc.p, el.p);
    CHECK(enc.host(s) == fb.vartime_multiscalar_mul(dk));
    CHECK(e.vartime_compress(el.host(s)) == enc.host(s));
    fb.msm_long_resident(0, s, k.p, 3, enc.p);
    const std::vector<Encoding> got = enc.host(s), want = fb.msm_long(std::vector<Fr>(dk.begin(), dk.begin() + 3 * m));
    CHECK(std::vector<Encoding>(got.begin(), got.begin() + 3) == want);
  }

  // the indexed and the mixed sums, with a clean index array and with a planted one
  std::vector<Fr> fk(n * t), vk(n * v);
  random_fr(fk); random_fr(vk);
  std::vector<int> idx(n * t);
  for (size_t p = 0; p < idx.size(); ++p) idx[p] = (p % 7 == 3) ? -1 : (int)(rng() % m);
  {
    DevBuf<int> di(idx);
    DevBuf<Fr> dfk(fk), dvk(vk);
    DevBuf<Element> dA(A);
    DevBuf<Encoding> enc(n);
    DevBuf<uint64_t> verdict(2);
    fb.msm_indexed_resident(0, s, di.p, dfk.p, t, n, enc.p, nullptr, verdict.p);
    CHECK(enc.host(s) == fb.msm_indexed(idx, fk, t));
    CHECK(verdict.host(s) == (std::vector<uint64_t>{0, UINT64_MAX}));
    fb.msm_mixed_resident(0, s, di.p, dfk.p, t, dA.p, dvk.p, v, n, enc.p, nullptr, verdict.p);
    CHECK(enc.host(s) == fb.msm_mixed(idx, fk, t, A, vk, v));
    CHECK(verdict.host(s) == (std::vector<uint64_t>{0, UINT64_MAX}));

    std::vector<int> bad(idx), mended(idx);
    bad[130] = (int)m; bad[400] = -2;
    mended[130] = mended[400] = -1;                            // a refused index contributes nothing
    DevBuf<int> dbad(bad);
    fb.msm_mixed_resident(0, s, dbad.p, dfk.p, t, dA.p, dvk.p, v, n, enc.p, nullptr, verdict.p);
    CHECK(enc.host(s) == fb.msm_mixed(mended, fk, t, A, vk, v));
    CHECK(verdict.host(s) == (std::vector<uint64_t>{2, 130}));
    fb.check_base_index_resident(0, s, dbad.p, bad.size(), verdict.p);
    CHECK(verdict.host(s) == (std::vector<uint64_t>{2, 130}));
    bool threw = false;                                        // a misaligned record buffer: refused by the library
    try { fb.msm_indexed_resident(0, s, di.p, reinterpret_cast<const Fr*>(reinterpret_cast<const uint8_t*>(dfk.p) + 4), t, n - 1, enc.p); }
    catch (const DeviceError&) { threw = true; }
    CHECK(threw);
  }

  HIP_OK(hipStreamDestroy(s));
  std::printf("CPP_RESIDENT_SUMS_OK\n");
  return 0;
}
#endif
