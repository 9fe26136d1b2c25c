// libcfdenoise: the inverse of a tie table as cfd_denoise_guide reads it (guide.hpp, guide_update_kernel).  Plain C++: no HIP header, no
// device code -- tests/host/guide_tables_test.cpp builds it alone.
//
// A tie table names, per token e of n = B * L, its source tie[e] (a flat token index) or -1 (a free token; cfd_sample_begin_tied,
// run_kind.check_tie: several tokens may share one source, a source is never tied itself, so the fold of gradients is one level deep).
// The inverse in CSR form, int32 [2 n + 1]:
//   csr[0 .. n]          offsets: the tokens tied to source s are csr[n + 1 + k] for k in [csr[s], csr[s + 1])
//   csr[n + 1 .. 2 n]    those tokens, ascending within a source (the order the fold sums in); entries beyond csr[n] are -1
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

enum { GUIDE_CSR_OK = 0, GUIDE_CSR_RANGE = 1, GUIDE_CSR_SELF = 2, GUIDE_CSR_CHAIN = 3 };

inline size_t guide_csr_len(long long n) { return (size_t)(2 * n + 1); }

// Fills csr (guide_csr_len(n) entries).  Returns GUIDE_CSR_OK, or why the table is no tie table, with the first offending token in *bad.
inline int guide_build_tie_csr(const int32_t* tie, long long n, int32_t* csr, long long* bad = nullptr) {
  auto refuse = [&](int why, long long e) { if (bad) *bad = e; return why; };
  for (long long e = 0; e < n; ++e) {
    const long long v = tie[e];
    if (v == -1) continue;
    if (v < -1 || v >= n) return refuse(GUIDE_CSR_RANGE, e);
    if (v == e) return refuse(GUIDE_CSR_SELF, e);
    if (tie[v] != -1) return refuse(GUIDE_CSR_CHAIN, e);
  }
  std::vector<int32_t> count((size_t)n + 1, 0);
  for (long long e = 0; e < n; ++e)
    if (tie[e] >= 0) ++count[(size_t)tie[e] + 1];
  csr[0] = 0;
  for (long long s = 0; s < n; ++s) csr[s + 1] = csr[s] + count[(size_t)s + 1];
  int32_t* list = csr + n + 1;
  for (long long k = 0; k < n; ++k) list[k] = -1;
  std::vector<int32_t> at(csr, csr + n);          // next free slot of every source
  for (long long e = 0; e < n; ++e)               // ascending e: ascending within a source
    if (tie[e] >= 0) list[at[(size_t)tie[e]]++] = (int32_t)e;
  return GUIDE_CSR_OK;
}
