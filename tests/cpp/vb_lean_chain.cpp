// Stand-alone host run of the variable-base kernels' chain (curve.hpp: ge_scalar_mul_w4_lean) for the sanitizers: built by
// tests/test_vb_lean_host.py with g++ -fsanitize=address,undefined and run as an ordinary program; nothing in
// decaf377_amd/ loads it.  It reads lines "S <encoding> <scalar>" (64 hex digits each) from standard input, runs
// k_scalar_mul_var's lane and k_scalar_mul_var_el's chain over the three host tables with the lean chain and with the
// reference statement ge_scalar_mul_w4<fes>, requires the two to agree byte for byte, and prints per input
//   "S <lane encoding> <lane status> <element-chain encoding> <status>"
// for the driver to compare with the oracle.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../host_sim/vb_lean_sim.cpp"

namespace {
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
}  // namespace

int main() {
  if (sim_init() != 0) { fprintf(stderr, "vb_lean_chain: sim_init failed\n"); return 2; }
  std::vector<uint32_t> enc, k;
  char buf[4096];
  while (fgets(buf, sizeof buf, stdin)) {
    std::string line(buf);
    while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
    if (line.empty()) continue;
    uint32_t a[8], b[8];
    if (line[0] != 'S' || line.size() != 2 + 64 + 1 + 64 || !hex_words(line.substr(2, 64), a) || !hex_words(line.substr(67, 64), b)) {
      fprintf(stderr, "vb_lean_chain: bad line: %s\n", line.c_str());
      return 2;
    }
    enc.insert(enc.end(), a, a + 8); k.insert(k.end(), b, b + 8);
  }
  const size_t n = enc.size() / 8;
  int failures = 0;
  std::vector<uint32_t> lane(8 * n), el(8 * n), o(8 * n);
  std::vector<uint8_t> lane_st(n), el_st(n), st(n);
  for (int table = 0; table < 3; ++table)
    for (int chain = 1; chain >= 0; --chain) {
      const bool first = table == 0 && chain == 1;
      unsigned long s0 = vbl_scalar_mul_var(chain, table, table == 1, enc.data(), k.data(), n, first ? lane.data() : o.data(), first ? lane_st.data() : st.data());
      if (!first && (o != lane || st != lane_st)) { fprintf(stderr, "vb_lean_chain: lane, table %d chain %d differs\n", table, chain); ++failures; }
      s0 += vbl_scalar_mul_var_sqrt(chain, table, enc.data(), k.data(), n, first ? el.data() : o.data(), first ? el_st.data() : st.data());
      if (!first && (o != el || st != el_st)) { fprintf(stderr, "vb_lean_chain: element chain, table %d chain %d differs\n", table, chain); ++failures; }
      if (table != 0 && s0 != 0) { fprintf(stderr, "vb_lean_chain: a shared-identity table was handed a store(0)\n"); ++failures; }
    }
  for (size_t i = 0; i < n; ++i)
    printf("S %s %d %s %d\n", words_hex(&lane[8 * i]).c_str(), (int)lane_st[i], words_hex(&el[8 * i]).c_str(), (int)el_st[i]);
  if (failures) { fprintf(stderr, "vb_lean_chain: %d check(s) failed\n", failures); return 1; }
  printf("OK\n");
  return 0;
}
