// host_check.cpp — drives libcgx's host-only code under AddressSanitizer and
// UndefinedBehaviorSanitizer (tests/sanitize/Makefile builds the host
// objects with -fsanitize=address,undefined; the device code is not
// instrumented). No GPU is touched. Covered:
//   * cgx_mm_read / cgx_mm_write_lower (cgx_mm.cpp) on every golden .mtx
//     (including the quirk files) at 1..8 threads, and a write/read round
//     trip;
//   * the SELL and SELL-P planners (cgx_sell_plan, cgx_sellp_plan) and the
//     row-block schedule (cgx_row_blocks) on Poisson, irregular, empty-row
//     and single-row matrices;
//   * the halo planners (cgx_plan_ghosts, cgx_plan_remap) on 1-D row
//     partitions of those matrices at 1..5 ranks;
//   * the SpMV variant resolution (launch_variant, launch_variant_ok,
//     spmv_listed: pure host functions of a CsrDev) over a fixed grid of
//     synthetic CsrDevs and a fixed request list, against the table
//     <golden dir>/spmv_variant_table.txt recorded from the commit before
//     the variant bits were named.
// Any sanitizer report aborts with a non-zero exit; the test checks exit 0.
//   host_check <golden dir> <tmp dir>
//   host_check --dump-variants     the full resolution table, for a diff
#include <cstdint>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "cgx.h"
#include "cgx_internal.h"

#define EXPECT(c)                                                        \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::fprintf(stderr, "FAILED %s at %s:%d\n", #c, __FILE__, __LINE__); \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

struct Csr {
  std::vector<int> rp, col;
  std::vector<double> val;
  int64_t n() const { return (int64_t)rp.size() - 1; }
};

static Csr poisson(int dim, int nx, int ny, int nz) {
  Csr m;
  m.rp.push_back(0);
  const long nxy = (long)nx * ny;
  for (long z = 0; z < (dim == 3 ? nz : 1); ++z)
    for (long y = 0; y < ny; ++y)
      for (long x = 0; x < nx; ++x) {
        const long r = x + nx * y + nxy * z;
        auto add = [&](long c, double v) { m.col.push_back((int)c); m.val.push_back(v); };
        if (dim == 3 && z > 0) add(r - nxy, -1);
        if (y > 0) add(r - nx, -1);
        if (x > 0) add(r - 1, -1);
        add(r, 2.0 * dim);
        if (x < nx - 1) add(r + 1, -1);
        if (y < ny - 1) add(r + nx, -1);
        if (dim == 3 && z < nz - 1) add(r + nxy, -1);
        m.rp.push_back((int)m.col.size());
      }
  return m;
}

// rows of 0..maxlen random distinct ascending columns (empty rows included)
static Csr irregular(int64_t n, int maxlen, uint64_t seed) {
  Csr m;
  m.rp.push_back(0);
  uint64_t s = seed;
  auto rnd = [&]() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return s >> 33; };
  for (int64_t r = 0; r < n; ++r) {
    const int len = (int)(rnd() % (maxlen + 1));
    std::vector<int> cs;
    for (int k = 0; k < len; ++k) {
      int64_t c = r + (int64_t)(rnd() % 2001) - 1000;
      if (c < 0) c = 0;
      if (c >= n) c = n - 1;
      cs.push_back((int)c);
    }
    std::sort(cs.begin(), cs.end());
    cs.erase(std::unique(cs.begin(), cs.end()), cs.end());
    for (int c : cs) { m.col.push_back(c); m.val.push_back(1.0 + (double)(rnd() % 7)); }
    m.rp.push_back((int)m.col.size());
  }
  return m;
}

static void plans(const Csr &m) {
  const int64_t n = m.n();
  int64_t nrb = 0;
  int *rb = nullptr;
  int mx = 0;
  EXPECT(cgx_row_blocks(m.rp.data(), n, &nrb, &rb, &mx) == CGX_OK);
  EXPECT(nrb >= 1 && rb[0] == 0 && rb[nrb] == n);
  cgx_free_host(rb);
  for (int R : {1, 2}) {
    int64_t nsl = 0, ndict = 0, nidx = 0, vs = 0;
    int64_t *sl = nullptr;
    int *dict = nullptr;
    unsigned long long *idx = nullptr;
    EXPECT(cgx_sell_plan(m.rp.data(), m.col.data(), n, R, &nsl, &sl, &ndict, &dict, &nidx, &idx,
                         &vs) == CGX_OK);
    cgx_free_host(sl);
    cgx_free_host(dict);
    cgx_free_host(idx);
  }
  int64_t nsl = 0, npat = 0, vs = 0;
  int64_t *sl = nullptr;
  int *pat = nullptr;
  int maxw = 0;
  EXPECT(cgx_sellp_plan(m.rp.data(), m.col.data(), n, &nsl, &sl, &npat, &pat, &vs, &maxw) ==
         CGX_OK);
  cgx_free_host(sl);
  cgx_free_host(pat);
  // halo plans of a 1-D row partition at 1..5 ranks
  for (int world = 1; world <= 5; ++world) {
    std::vector<int64_t> begins(world), counts(world);
    for (int r = 0; r < world; ++r) {
      begins[r] = n * r / world;
      counts[r] = n * (r + 1) / world - begins[r];
    }
    for (int r = 0; r < world; ++r) {
      const int64_t b = begins[r], c = counts[r];
      if (c == 0) continue;
      std::vector<int> cols(m.col.begin() + m.rp[b], m.col.begin() + m.rp[b + c]);
      int64_t ng = 0;
      int64_t *gh = nullptr;
      std::vector<int64_t> recv(world);
      EXPECT(cgx_plan_ghosts(c, b, (int64_t)cols.size(), cols.data(), world, begins.data(),
                             counts.data(), &ng, &gh, recv.data()) == CGX_OK);
      int64_t tot = 0;
      for (int64_t v : recv) tot += v;
      EXPECT(tot == ng);
      EXPECT(cgx_plan_remap(c, b, (int64_t)cols.size(), cols.data(), ng, gh) == CGX_OK);
      for (int v : cols) EXPECT(v >= 0 && v < c + ng);
      cgx_free_host(gh);
    }
  }
}

// ---- SpMV variant resolution ------------------------------------------------
// The requests, as the public decimals (on purpose not the library's names):
// every form the list held before the names, with the four retired y-march
// numbers; the request forms cgx_csr_set_variant listed; the tuning
// ablations; unknown and retired bits; the value-code forms with 2^24 set.
static const int kRequests[] = {
    0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15, 264, 265, 266, 133, 135, 67108877, 67108879, 267,
    2048, 2050, 2056, 2058, 6144, 6146, 8192, 8194, 24576, 24578, 40960, 40962, 303104, 303106,
    565248, 565250, 827392, 827394, 1613824, 1613826, 1875968, 1875970, 3710976, 3710978,
    3973120, 3973122, 9216000, 9216002, 10264576, 10264578, 12361728, 12361730,
    20750336, 20750338, 29138944, 29138946,
    34816, 34818, 296960, 296962, 559104, 559106, 821248, 821250, 1607680, 1607682, 1869824,
    1869826, 9209856, 9209858, 10258434, 12355584, 12355586, 10258432,
    31, 47, 63, 67108927, 67108911,
    64, 512, 9999, 2138112,
    16818176, 16818178, 17080320, 17080322, 17342464, 17342466, 17604608, 17604610, 18391040,
    18391042, 18653184, 18653186, 20488192, 20488194, 25993216, 25993218, 27041792, 27041794};
constexpr int kListed = 56;  // the leading entries: the list before the names
static bool retired(int v) {
  return v == 20750336 || v == 20750338 || v == 29138944 || v == 29138946;
}

struct VariantCfg {
  int sl, kind, r, vc, maxw, march, tmpl, off;
  long long nnz;
  int f64;
};

// the configuration's line, its hash last; `full`: every (request,
// resolved variant, has a kernel) after it
static std::string variant_row(const VariantCfg &c, bool full) {
  alignas(64) static char buf[256];
  cgx::CsrDev A{};
  A.n = 100;
  A.nnz = c.nnz;
  A.val = buf + c.off;
  A.col = (const int *)(buf + 64 + c.off);
  if (c.sl) {
    A.sl = (const cgx::SellSlice *)buf;
    A.sell_kind = c.kind;
    A.sell_r = c.r;
    A.svc = c.vc >= 1 ? buf : nullptr;
    A.svc4 = c.vc >= 2 ? buf : nullptr;
    A.sell_maxw = c.maxw;
    A.march_k = c.march;
    if (c.tmpl) {
      A.sl_t = (const cgx::SellSlice *)buf;
      A.vct = buf;
      A.nvt = 2;
    }
  }
  A.col16 = (const short *)buf;
  A.il = buf;
  A.lean = false;
  const int dt = c.f64 ? CGX_F64 : CGX_F32;
  uint64_t h = 14695981039346656037ull;  // FNV-1a, the two ints byte by byte
  auto fold = [&](unsigned v) {
    for (int b = 0; b < 4; ++b) h = (h ^ ((v >> (8 * b)) & 0xffu)) * 1099511628211ull;
  };
  std::string rest;
  char t[64];
  for (int q : kRequests) {
    A.variant = q;
    const int v = cgx::launch_variant(A, dt);
    const int ok = cgx::launch_variant_ok(A, dt) ? 1 : 0;
    fold((unsigned)v);
    fold((unsigned)ok);
    if (full) {
      std::snprintf(t, sizeof t, " %d:%d:%d", q, v, ok);
      rest += t;
    }
  }
  char line[200];
  std::snprintf(line, sizeof line,
                "sl=%d kind=%d r=%d vc=%d maxw=%d march=%d tmpl=%d off=%d nnz=%lld %s %016llx",
                c.sl, c.kind, c.r, c.vc, c.maxw, c.march, c.tmpl, c.off, c.nnz,
                c.f64 ? "f64" : "f32", (unsigned long long)h);
  return line + rest;
}

// the SELL fields (and the templates on them) count only when sl is set
static std::vector<VariantCfg> variant_grid() {
  std::vector<VariantCfg> g;
  for (int sl : {0, 1})
    for (int kind : {0, 1, 2})
      for (int r : {1, 2})
        for (int vc : {0, 1, 2})
          for (int maxw : {7, 9})
            for (int march : {0, 2})
              for (int tmpl : {0, 1}) {
                if (!sl && (kind != 0 || r != 1 || vc != 0 || maxw != 7 || march != 0 || tmpl))
                  continue;
                for (int off : {0, 8, 4})
                  for (long long nnz : {1ll, 3ll, 1000ll})
                    for (int f64 : {0, 1})
                      g.push_back({sl, kind, r, vc, maxw, march, tmpl, off, nnz, f64});
              }
  return g;
}

static void variant_dump() {
  for (const VariantCfg &c : variant_grid()) std::printf("%s\n", variant_row(c, true).c_str());
}

static void variant_table(const std::string &gold) {
  for (int k = 0; k < (int)(sizeof kRequests / sizeof kRequests[0]); ++k) {
    const int v = kRequests[k];
    if (k < kListed) EXPECT(cgx::spmv_listed(v) == !retired(v));
  }
  std::FILE *f = std::fopen((gold + "/spmv_variant_table.txt").c_str(), "r");
  EXPECT(f != nullptr);
  char line[256];
  size_t bad = 0, rows = 0;
  for (const VariantCfg &c : variant_grid()) {
    EXPECT(std::fgets(line, sizeof line, f) != nullptr);
    std::string want = line;
    while (!want.empty() && (want.back() == '\n' || want.back() == '\r')) want.pop_back();
    ++rows;
    if (variant_row(c, false) == want) continue;
    if (++bad <= 10)
      std::fprintf(stderr, "variant table: recorded %s\n  now %s\n", want.c_str(),
                   variant_row(c, true).c_str());
  }
  EXPECT(std::fgets(line, sizeof line, f) == nullptr);  // no row left over
  std::fclose(f);
  if (bad) std::fprintf(stderr, "variant table: %zu of %zu rows differ\n", bad, rows);
  EXPECT(bad == 0);
}

int main(int argc, char **argv) {
  if (argc == 2 && std::string(argv[1]) == "--dump-variants") {
    variant_dump();
    return 0;
  }
  if (argc < 3) return 2;
  const std::string gold = argv[1], tmp = argv[2];
  const char *files[] = {"poisson2d_16.mtx", "poisson2d_128.mtx", "poisson3d_16.mtx",
                         "quirks_emptyrow.mtx", "quirks_general.mtx", "quirks_nocomment.mtx"};
  for (const char *f : files) {
    for (int threads : {1, 3, 8}) {
      int64_t n = 0, nnz = 0;
      int *rp = nullptr, *col = nullptr;
      double *val = nullptr;
      EXPECT(cgx_mm_read((gold + "/" + f).c_str(), threads, &n, &nnz, &rp, &col, &val) == CGX_OK);
      Csr m;
      m.rp.assign(rp, rp + n + 1);
      m.col.assign(col, col + nnz);
      m.val.assign(val, val + nnz);
      cgx_free_host(rp);
      cgx_free_host(col);
      cgx_free_host(val);
      // the quirk files keep the loader's Q3 behaviour (empty rows dropped, so
      // columns may point past N): no partition owns those columns
      if (threads == 1 && std::string(f).rfind("quirks", 0) != 0) plans(m);
    }
  }
  // write / read round trip of a symmetric matrix
  Csr p = poisson(3, 9, 7, 5);
  const std::string out = tmp + "/rt.mtx";
  EXPECT(cgx_mm_write_lower(out.c_str(), p.n(), p.rp.data(), p.col.data(), p.val.data(), 4) ==
         CGX_OK);
  int64_t n = 0, nnz = 0;
  int *rp = nullptr, *col = nullptr;
  double *val = nullptr;
  EXPECT(cgx_mm_read(out.c_str(), 4, &n, &nnz, &rp, &col, &val) == CGX_OK);
  EXPECT(n == p.n() && nnz == (int64_t)p.val.size());
  for (int64_t k = 0; k < nnz; ++k) EXPECT(col[k] == p.col[k] && val[k] == p.val[k]);
  cgx_free_host(rp);
  cgx_free_host(col);
  cgx_free_host(val);
  // a missing file is an error, not a crash
  EXPECT(cgx_mm_read((tmp + "/missing.mtx").c_str(), 2, &n, &nnz, &rp, &col, &val) != CGX_OK);
  plans(poisson(2, 130, 70, 1));
  plans(poisson(3, 33, 17, 9));
  plans(irregular(20000, 40, 1));
  plans(irregular(3000, 200, 2));
  plans(poisson(2, 1, 1, 1));
  variant_table(gold);
  std::printf("host_check ok\n");
  return 0;
}
