// Host test of csrc/guide_tables.hpp (the inverse tie table of cfd_denoise_guide) and of the row limit a caller passes to
// decide_forward_path (csrc/forward_path.hpp, PathAsk::max_rows).  Expected values are written out by hand.  Built with the host
// compiler under AddressSanitizer and UBSan by tests/test_guide_tables_host.py; exit status 0 = every check held.
#include "../../convofusion_amd/csrc/forward_path.hpp"
#include "../../convofusion_amd/csrc/guide_tables.hpp"

#include <cstdio>
#include <vector>

static int bad = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++bad; } \
  } while (0)

static PathShape shape(int Be, int L, int audio = 20) {
  PathShape s;
  s.Be = Be; s.L = L; s.tmode = 0;
  const int S[FP_NMEM] = {6, audio, 6, 8, 1};
  for (int j = 0; j < FP_NMEM; ++j) s.S[j] = S[j];
  return s;
}

static bool same_path(const ForwardPath& g, const ForwardPath& w) {
  return g.rt == w.rt && g.xattn == w.xattn && g.xa_inst == w.xa_inst && g.xa_list == w.xa_list && g.f16_mask == w.f16_mask && g.share == w.share &&
         g.share_rows == w.share_rows && g.ln_fold == w.ln_fold && g.rows_now == w.rows_now && g.dstep_slot == w.dstep_slot &&
         g.static_mask == w.static_mask && g.xa_reached == w.xa_reached;
}

static void csr_checks() {
  {   // three windows of four tokens: the first half of window w is tied to the second half of window w - 1
    const std::vector<int32_t> tie = {-1, -1, -1, -1, 2, 3, -1, -1, 6, 7, -1, -1};
    const long long n = (long long)tie.size();
    std::vector<int32_t> csr(guide_csr_len(n), 12345);
    EXPECT(guide_csr_len(n) == 25);
    EXPECT(guide_build_tie_csr(tie.data(), n, csr.data()) == GUIDE_CSR_OK);
    const std::vector<int32_t> off = {0, 0, 0, 1, 2, 2, 2, 3, 4, 4, 4, 4, 4};
    const std::vector<int32_t> list = {4, 5, 8, 9, -1, -1, -1, -1, -1, -1, -1, -1};
    EXPECT(std::vector<int32_t>(csr.begin(), csr.begin() + 13) == off);
    EXPECT(std::vector<int32_t>(csr.begin() + 13, csr.end()) == list);
  }
  {   // several tokens on one source, given out of order by source: ascending within a source
    const std::vector<int32_t> tie = {5, -1, 1, 5, 1, -1, 5};
    const long long n = (long long)tie.size();
    std::vector<int32_t> csr(guide_csr_len(n), 12345);
    EXPECT(guide_build_tie_csr(tie.data(), n, csr.data()) == GUIDE_CSR_OK);
    const std::vector<int32_t> off = {0, 0, 2, 2, 2, 2, 5, 5};
    const std::vector<int32_t> list = {2, 4, 0, 3, 6, -1, -1};
    EXPECT(std::vector<int32_t>(csr.begin(), csr.begin() + 8) == off);
    EXPECT(std::vector<int32_t>(csr.begin() + 8, csr.end()) == list);
  }
  {   // no ties, one token
    const int32_t tie[1] = {-1};
    int32_t csr[3] = {9, 9, 9};
    EXPECT(guide_build_tie_csr(tie, 1, csr) == GUIDE_CSR_OK);
    EXPECT(csr[0] == 0 && csr[1] == 0 && csr[2] == -1);
  }
  {   // refusals, with the first offending token; nothing is written past the table
    long long at = -1;
    std::vector<int32_t> csr(guide_csr_len(3));
    const int32_t range[3] = {-1, 3, -1}, below[3] = {-2, -1, -1}, self[3] = {-1, -1, 2}, chain[3] = {1, 2, -1};
    EXPECT(guide_build_tie_csr(range, 3, csr.data(), &at) == GUIDE_CSR_RANGE && at == 1);
    EXPECT(guide_build_tie_csr(below, 3, csr.data(), &at) == GUIDE_CSR_RANGE && at == 0);
    EXPECT(guide_build_tie_csr(self, 3, csr.data(), &at) == GUIDE_CSR_SELF && at == 2);
    EXPECT(guide_build_tie_csr(chain, 3, csr.data(), &at) == GUIDE_CSR_CHAIN && at == 0);
    EXPECT(guide_build_tie_csr(chain, 3, csr.data()) == GUIDE_CSR_CHAIN);
  }
}

static void row_limit_checks() {
  const PathKnobs dflt;
  PathAsk plain, guide;
  guide.max_rows = 4096;
  EXPECT(plain.max_rows == 0);
  // the default ask reproduces today's decisions on the shapes of tests/host/forward_path_test.cpp's table around the row limit
  EXPECT(decide_forward_path(dflt, shape(14, 16), plain).rt);
  EXPECT(decide_forward_path(dflt, shape(25, 28), plain).rt);            // 700 rows exactly stay
  const ForwardPath over = decide_forward_path(dflt, shape(44, 16), plain);   // 704 > 700: the fused kernel, the fold's range
  EXPECT(!over.rt && over.xattn == XATTN_FUSED && over.xa_inst == XA_INST_PAIR && over.xa_list && over.ln_fold && over.static_mask == 31);
  // a caller's own limit stands in place of the knob's: 704, 768, 1440 and 4096 rows stay on the row-tile path, 4112 do not
  for (int Be : {44, 48, 90, 256}) {
    const ForwardPath p = decide_forward_path(dflt, shape(Be, 16), guide);
    EXPECT(p.rt && p.xattn == XATTN_ROWTILE && p.xa_inst == XA_INST_NONE && !p.ln_fold && p.static_mask == 31);
  }
  EXPECT(!decide_forward_path(dflt, shape(257, 16), guide).rt);
  // ... and moves nothing else: below the knob's limit the two asks decide alike, and the knob itself does not bound the caller's limit
  EXPECT(same_path(decide_forward_path(dflt, shape(14, 16), plain), decide_forward_path(dflt, shape(14, 16), guide)));
  PathKnobs low = dflt;
  low.rt_max_rows = 100;
  EXPECT(!decide_forward_path(low, shape(14, 16), plain).rt && decide_forward_path(low, shape(14, 16), guide).rt);
  // the other limits of the row-tile path stay: L, the padded keys, the switch, a dynamic memory
  EXPECT(!decide_forward_path(dflt, shape(2, 34), guide).rt);
  EXPECT(!decide_forward_path(dflt, shape(14, 16, 1000), guide).rt);
  PathKnobs off = dflt;
  off.rt_on = false;
  EXPECT(!decide_forward_path(off, shape(14, 16), guide).rt);
  PathAsk dyn = guide;
  dyn.dynamic_mask = 16;
  EXPECT(!decide_forward_path(dflt, shape(14, 16), dyn).rt);
}

int main() {
  csr_checks();
  row_limit_checks();
  if (bad) {
    printf("%d checks failed\n", bad);
    return 1;
  }
  printf("all checks passed\n");
  return 0;
}
