// nmod_write_sign_test and nmod_format_probe: save_test's table (myDetect.py:532-536), buffered.  Plain host C++: no HIP
// header and no device code, so that this unit can be built and exercised on its own.
//
// '%.3f' and '%.3E' exactly as printf (and Python) round them — the exact binary value, half to even — without going
// through printf for every number (350 ns each: the table writer was the largest piece of a 4.6 M-position mtest2).
// x87 extended precision carries 64 bits: |v| * 1000 is exact in it for every double below 2^63 / 1000, so '%.3f' is
// decided exactly; '%.3E' scales by a power of ten (relative error ~2^-62) and hands every value whose fourth
// significant digit is within 1e-7 of a rounding boundary to snprintf.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <thread>
#include <vector>

#include "../../include/nanomod_hip.h"

static_assert(sizeof(long double) >= 10 && __LDBL_MANT_DIG__ >= 64, "the fast formats need a 64-bit significand");

static inline char* put_digits(char* p, unsigned long long v) {
  char tmp[24]; int n = 0;
  do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
  while (n) *p++ = tmp[--n];
  return p;
}
static inline char* put_3(char* p, unsigned v) { p[0] = (char)('0' + v / 100); p[1] = (char)('0' + v / 10 % 10); p[2] = (char)('0' + v % 10); return p + 3; }
static inline char* put_f3(char* p, double v) {          // '%.3f' as Python formats it
  if (v != v) { memcpy(p, "nan", 3); return p + 3; }
  if (v == INFINITY) { memcpy(p, "inf", 3); return p + 3; }
  if (v == -INFINITY) { memcpy(p, "-inf", 4); return p + 4; }
  const double a = fabs(v);
  if (!(a < 9.0e15)) return p + snprintf(p, 400, "%.3f", v);
  const long double x = (long double)a * 1000.0L;         // exact: 53 + 10 bits
  unsigned long long d = (unsigned long long)x;           // truncation
  const long double frac = x - (long double)d;            // exact
  if (frac > 0.5L || (frac == 0.5L && (d & 1ull))) ++d;   // half to even on the exact value
  if (signbit(v)) *p++ = '-';
  p = put_digits(p, d / 1000);
  *p++ = '.';
  return put_3(p, (unsigned)(d % 1000));
}
struct Pow10Table {                                       // 10^i, i = -360 .. 360, as long double
  long double v[721];
  Pow10Table() { for (int i = 0; i <= 720; ++i) v[i] = powl(10.0L, (long double)(i - 360)); }
  long double operator()(int i) const { return v[i + 360]; }
};
static inline char* put_e3(char* p, double v) {          // '%.3E'
  static const Pow10Table pow10;
  if (v != v) { memcpy(p, "NAN", 3); return p + 3; }      // Python upper-cases non-finite values under %E
  if (v == INFINITY) { memcpy(p, "INF", 3); return p + 3; }
  if (v == -INFINITY) { memcpy(p, "-INF", 4); return p + 4; }
  const double a = fabs(v);
  if (a == 0.0) { if (signbit(v)) *p++ = '-'; memcpy(p, "0.000E+00", 9); return p + 9; }
  int e2;
  frexp(a, &e2);                                          // a = f * 2^e2, 0.5 <= f < 1
  int k = (int)floor((e2 - 1) * 0.30102999566398120);     // floor(log10 a) or one less
  long double x = (long double)a * pow10(3 - k);          // want 1000 <= x < 10000
  if (x >= 10000.0L) { ++k; x = (long double)a * pow10(3 - k); }
  else if (x < 1000.0L) { --k; x = (long double)a * pow10(3 - k); }
  if (!(x >= 1000.0L && x < 10000.0L)) return p + snprintf(p, 64, "%.3E", v);
  unsigned d = (unsigned)x;
  const long double frac = x - (long double)d;
  // (near a boundary of the fourth digit — or of the power of ten itself — the scaled value is not trusted)
  if (fabsl(frac - 0.5L) < 1e-7L || frac < 1e-7L || frac > 1.0L - 1e-7L) return p + snprintf(p, 64, "%.3E", v);
  if (frac > 0.5L) ++d;
  if (d == 10000u) { d = 1000u; ++k; }
  if (signbit(v)) *p++ = '-';
  *p++ = (char)('0' + d / 1000); *p++ = '.';
  p = put_3(p, d % 1000);
  *p++ = 'E'; *p++ = k < 0 ? '-' : '+';
  const unsigned ak = (unsigned)(k < 0 ? -k : k);
  if (ak >= 100) { return put_3(p, ak); }
  p[0] = (char)('0' + ak / 10); p[1] = (char)('0' + ak % 10);
  return p + 2;
}

extern "C" {

// test hook: the two formats on an array of values, NUL-separated (tests/test_abi_and_host.py compares with Python)
int nmod_format_probe(const double* v, int64_t n, int32_t sci, char* out, int64_t cap) {
  if (!v || !out || n < 0) return NMOD_ERR_INVALID_ARG;
  char* p = out;
  for (int64_t i = 0; i < n; ++i) {
    if (p - out + 420 > cap) return NMOD_ERR_INVALID_ARG;
    p = sci ? put_e3(p, v[i]) : put_f3(p, v[i]);
    *p++ = '\0';
  }
  return NMOD_OK;
}

int nmod_write_sign_test(const char* path, int64_t npos, const int32_t* chrom_id, const char* chrom_names,
                         int32_t n_chroms, const char* strand, const int64_t* pos0, const char* base,
                         const int32_t* n0, const int32_t* n1, const double* mwu_u, const double* mwu_p,
                         const double* t_t, const double* t_p, const double* ks_d, const double* ks_p,
                         const double* comb_st, const double* comb_p, int32_t with_comb) {
  if (!path || npos < 0 || n_chroms < 0) return NMOD_ERR_INVALID_ARG;
  if (npos > 0 && (!chrom_id || !chrom_names || !strand || !pos0 || !base || !n0 || !n1 || !mwu_u || !mwu_p || !t_t ||
                   !t_p || !ks_d || !ks_p || (with_comb && (!comb_st || !comb_p)))) return NMOD_ERR_INVALID_ARG;
  std::vector<const char*> names(n_chroms);
  size_t longest = 0;
  const char* q = chrom_names;
  std::vector<size_t> name_len(n_chroms);
  for (int i = 0; i < n_chroms; ++i) { names[i] = q; name_len[i] = strlen(q); longest = std::max(longest, name_len[i]); q += name_len[i] + 1; }
  for (int64_t i = 0; i < npos; ++i) if (chrom_id[i] < 0 || chrom_id[i] >= n_chroms) return NMOD_ERR_INVALID_ARG;
  FILE* f = fopen(path, "w");
  if (!f) return NMOD_ERR_INVALID_ARG;
  // lines are formatted by several host threads, a block of positions each, and written in order
  const size_t line_cap = longest + 4096;              // '%.3f' of a value near DBL_MAX prints ~310 digits, eight of them never do
  auto format_block = [&](int64_t lo, int64_t hi, std::vector<char>& buf) {
    buf.clear();
    buf.reserve((size_t)(hi - lo) * 160);
    std::vector<char> line(line_cap);
    for (int64_t i = lo; i < hi; ++i) {
      char* p = line.data();
      {                                                       // "%s %c %lld %c %d %d "
        const char* nm = names[chrom_id[i]];
        const size_t ln = name_len[chrom_id[i]];
        memcpy(p, nm, ln); p += ln;
        *p++ = ' '; *p++ = strand[i]; *p++ = ' ';
        const long long ps = (long long)(pos0[i] + 1);
        if (ps < 0) { *p++ = '-'; p = put_digits(p, 0ull - (unsigned long long)ps); } else p = put_digits(p, (unsigned long long)ps);
        *p++ = ' '; *p++ = base[i]; *p++ = ' ';
        if (n0[i] < 0) { *p++ = '-'; p = put_digits(p, (unsigned long long)(-(long long)n0[i])); } else p = put_digits(p, (unsigned long long)n0[i]);
        *p++ = ' ';
        if (n1[i] < 0) { *p++ = '-'; p = put_digits(p, (unsigned long long)(-(long long)n1[i])); } else p = put_digits(p, (unsigned long long)n1[i]);
        *p++ = ' ';
      }
      p = put_f3(p, mwu_u[i]); *p++ = ' '; p = put_e3(p, mwu_p[i]); *p++ = ' ';
      p = put_f3(p, t_t[i]); *p++ = ' '; p = put_e3(p, t_p[i]); *p++ = ' ';
      p = put_f3(p, ks_d[i]); *p++ = ' '; p = put_e3(p, ks_p[i]);
      if (with_comb) { *p++ = ' '; p = put_f3(p, comb_st[i]); *p++ = ' '; p = put_e3(p, comb_p[i]); }
      *p++ = '\n';
      buf.insert(buf.end(), line.data(), p);
    }
  };
  const int64_t kBlock = 1 << 16;
  unsigned hw = std::thread::hardware_concurrency();
  const int nthreads = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)(hw ? hw : 1), 16, (npos + kBlock - 1) / kBlock}));
  bool ok = true;
  std::vector<std::vector<char>> bufs(nthreads);
  for (int64_t base_pos = 0; base_pos < npos && ok; base_pos += kBlock * nthreads) {
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t) {
      const int64_t lo = base_pos + (int64_t)t * kBlock, hi = std::min(npos, lo + kBlock);
      if (lo >= npos) { bufs[t].clear(); continue; }
      if (nthreads == 1) format_block(lo, hi, bufs[t]);
      else th.emplace_back(format_block, lo, hi, std::ref(bufs[t]));
    }
    for (auto& x : th) x.join();
    for (int t = 0; t < nthreads && ok; ++t)
      if (!bufs[t].empty()) ok = fwrite(bufs[t].data(), 1, bufs[t].size(), f) == bufs[t].size();
  }
  const bool closed = fclose(f) == 0;
  return (ok && closed) ? NMOD_OK : NMOD_ERR_INVALID_ARG;
}

}  // extern "C"
