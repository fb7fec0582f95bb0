// Stand-alone host check of the variable-base window table's packed slots (fqs29.hpp: fes_pack256 / fes_unpack256;
// d377.hip GlobalTab keeps four of them per 128-byte entry).  Built by tests/test_vb_packed_table_host.py with g++ -- plain,
// with -fsanitize=address,undefined, and with -DD377_BOUNDS -- and run as an ordinary program; nothing in decaf377_amd/
// loads it.  It reads commands from standard input, one per line, and answers each with one line:
//   P l0 .. l8            nine signed limbs       -> "P" the 8 packed words, then the 9 unpacked limbs
//   D enc digits          a 32-byte encoding and the 64 window digits as 8 words of nibbles (hex, word 0 first)
//                         -> "D" [sum d_i 16^i] P through ge_scalar_mul_w4<fes>: packed table, limb table (encodings)
//   S enc scalar          -> "S" k_scalar_mul_var's lane (decompression and window loop on fes, k halved, the compressor
//                            without a square root) and k_scalar_mul_var_el's chain, both over the packed table, and the
//                            first again over the limb table: encoding status, three times
// The program checks by itself what needs no big integers (limb ranges, packed table = limb table); the driver checks the
// values.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../host_sim/vb_signed_sqrt_sim.cpp"

namespace {
int g_failures = 0;
void require(bool ok, const char* what) {
  if (!ok) { fprintf(stderr, "vb_packed_table: %s\n", what); ++g_failures; }
}

// d377.hip GlobalTab on the host: [entry][4 slots x 8 words], entry 0 the one shared packed identity that nobody stores;
// a negative digit swaps the ypx / ymx slots by address
unsigned long g_packed_store0 = 0;
struct HostTabPacked {
  static constexpr bool shared_identity = true;
  uint32_t e[9][4 * PACKED_WORDS];
  HostTabPacked() {
    const gec_of<fes> id = gec_identity<fes>();
    put(0, id);
  }
  void put(int j, const gec_of<fes>& g) {
    fes_pack256(g.ypx, e[j]); fes_pack256(g.ymx, e[j] + PACKED_WORDS);
    fes_pack256(g.z2, e[j] + 2 * PACKED_WORDS); fes_pack256(g.kt, e[j] + 3 * PACKED_WORDS);
  }
  void store(int j, const gec_of<fes>& g) {
    if (j == 0) { ++g_packed_store0; return; }
    put(j, g);
  }
  gec_of<fes> load(int j, bool swap) const {
    const uint32_t* p = e[j];
    gec_of<fes> c;
    c.ypx = fes_unpack256(p + (swap ? PACKED_WORDS : 0));
    c.ymx = fes_unpack256(p + (swap ? 0 : PACKED_WORDS));
    c.z2 = fes_unpack256(p + 2 * PACKED_WORDS);
    c.kt = fes_unpack256(p + 3 * PACKED_WORDS);
    return c;
  }
};

void check_unpacked(const fes& u) {
  for (int i = 0; i < NL - 1; ++i) require(u.l[i] >= 0 && u.l[i] < (1 << 29), "unpacked limb outside [0, 2^29)");
  require(u.l[NL - 1] >= 0 && u.l[NL - 1] < (1 << 24), "unpacked top limb outside [0, 2^24)");
}

bool hex_words(const std::string& s, uint32_t w[8]) {   // 64 hex digits = 32 bytes, little-endian words
  if (s.size() != 64) return false;
  uint8_t b[32];
  for (int i = 0; i < 32; ++i) b[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
  memcpy(w, b, 32);
  return true;
}
std::string words_hex(const uint32_t w[8]) {
  uint8_t b[32]; memcpy(b, w, 32);
  char t[65];
  for (int i = 0; i < 32; ++i) snprintf(t + 2 * i, 3, "%02x", b[i]);
  return std::string(t);
}

void do_pack(const int32_t l[NL]) {
  fes a;
  for (int i = 0; i < NL; ++i) a.l[i] = l[i];
#if defined(D377_BOUNDS)
  double v = 0;                                            // the value in units of q, from the limbs themselves
  for (int i = 0; i < NL; ++i) { a.lo[i] = a.hi[i] = l[i]; v = v / 536870912.0 + (double)l[i]; }
  v /= Q_TOP;
  a.vlo = v - 1e-9; a.vhi = v + 1e-9;
#endif
  uint32_t w[PACKED_WORDS];
  fes_pack256(a, w);
  const fes u = fes_unpack256(w);
  check_unpacked(u);
  printf("P");
  for (int j = 0; j < PACKED_WORDS; ++j) printf(" %08" PRIx32, w[j]);
  for (int i = 0; i < NL; ++i) printf(" %" PRId32, u.l[i]);
  printf("\n");
}

void do_digits(const uint32_t enc[8], const uint32_t dg[8]) {
  RegPowTab pt; ge g;
  const uint32_t bad = ge_decompress(g_T, pt, enc, &g);
  require(bad == 0, "D: the encoding must be valid");
  uint32_t o1[8] = {0}, o2[8] = {0};
  if (!bad) {
    HostTabPacked tp; const ge r1 = ge_scalar_mul_w4<fes>(g, dg, tp);
    HostTabSharedId tu; const ge r2 = ge_scalar_mul_w4<fes>(g, dg, tu);
    ge_compress(g_T, pt, r1, o1); ge_compress(g_T, pt, r2, o2);
  }
  require(memcmp(o1, o2, 32) == 0, "D: packed table and limb table disagree");
  printf("D %s %s\n", words_hex(o1).c_str(), words_hex(o2).c_str());
}

// k_scalar_mul_var's lane over the table type Tab (tests/host_sim/vb_signed_sqrt_sim.cpp: vss_scalar_mul_var)
template <class Tab>
void lane_var(const std::vector<uint32_t>& enc, const std::vector<uint32_t>& k, size_t n, std::vector<uint32_t>& out, std::vector<uint8_t>& st) {
  dcb_rounds<1>(n, out.data(), true,
    [&](HostDcbIO& io, size_t i, int j) { dcb_put_den(io, 0, j, ge_decompress_den(enc.data() + 8 * i)); },
    [&](HostDcbIO& io, size_t i, int j) {
      const fe inv = dcb_get_inv(io, 0, j);
      RegPowTabS pt; ge g; const uint32_t bad = ge_decompress<fes>(g_T, pt, enc.data() + 8 * i, &g, &inv);
      st[i] = (uint8_t)bad;
      uint32_t kk[8], dg[8]; memcpy(kk, k.data() + 8 * i, 32); fr_reduce_words(kk); fr_half_words(kk); fr_recode_signed16(kk, dg);
      Tab tab; const ge r = ge_scalar_mul_w4<fes>(g, dg, tab, DCB_WANT_T);
      dcb_put(io, j, ge_dcb_from_half(r, bad != 0));
    });
}
void lane_el(const std::vector<uint32_t>& enc, const std::vector<uint32_t>& k, size_t n, std::vector<uint32_t>& out, std::vector<uint8_t>& st) {
  for (size_t i = 0; i < n; ++i) {
    RegPowTab pt; ge g; const uint32_t bad = ge_decompress(g_T, pt, enc.data() + 8 * i, &g);
    st[i] = (uint8_t)bad;
    if (bad) { memset(out.data() + 8 * i, 0, 32); continue; }
    uint32_t kk[8], dg[8]; memcpy(kk, k.data() + 8 * i, 32); fr_reduce_words(kk); fr_recode_signed16(kk, dg);
    HostTabPacked tab; const ge r = ge_scalar_mul_w4<fes>(g, dg, tab);
    ge_compress(g_T, pt, r, out.data() + 8 * i);
  }
}
}  // namespace

int main() {
  if (sim_init() != 0) { fprintf(stderr, "vb_packed_table: sim_init failed\n"); return 2; }
  std::vector<uint32_t> s_enc, s_k;
  char buf[4096];
  while (fgets(buf, sizeof buf, stdin)) {
    std::string line(buf);
    while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
    if (line.empty()) continue;
    if (line[0] == 'P') {
      int32_t l[NL];
      const char* p = line.c_str() + 1;
      char* end;
      for (int i = 0; i < NL; ++i) { l[i] = (int32_t)strtol(p, &end, 10); p = end; }
      do_pack(l);
    } else if (line[0] == 'D' || line[0] == 'S') {
      uint32_t a[8], b[8];
      if (line.size() != 2 + 64 + 1 + 64 || !hex_words(line.substr(2, 64), a) || !hex_words(line.substr(67, 64), b)) {
        fprintf(stderr, "vb_packed_table: bad line: %s\n", line.c_str());
        return 2;
      }
      if (line[0] == 'D') do_digits(a, b);
      else { s_enc.insert(s_enc.end(), a, a + 8); s_k.insert(s_k.end(), b, b + 8); }
    } else {
      fprintf(stderr, "vb_packed_table: unknown command: %s\n", line.c_str());
      return 2;
    }
  }
  const size_t n = s_enc.size() / 8;
  if (n) {
    std::vector<uint32_t> o1(8 * n), o2(8 * n), o3(8 * n);
    std::vector<uint8_t> t1(n), t2(n), t3(n);
    lane_var<HostTabPacked>(s_enc, s_k, n, o1, t1);
    lane_el(s_enc, s_k, n, o2, t2);
    lane_var<HostTabSharedId>(s_enc, s_k, n, o3, t3);
    for (size_t i = 0; i < n; ++i) {
      require(memcmp(&o1[8 * i], &o3[8 * i], 32) == 0 && t1[i] == t3[i], "S: packed table and limb table disagree");
      printf("S %s %d %s %d %s %d\n", words_hex(&o1[8 * i]).c_str(), (int)t1[i], words_hex(&o2[8 * i]).c_str(), (int)t2[i],
             words_hex(&o3[8 * i]).c_str(), (int)t3[i]);
    }
  }
  require(g_packed_store0 == 0, "the packed table was handed a store(0)");
  if (g_failures) { fprintf(stderr, "vb_packed_table: %d check(s) failed\n", g_failures); return 1; }
  printf("OK\n");
  return 0;
}
