// Host test of csrc/owned.hpp (DBuf, ArenaLayout, carve, GraphExec, HIPCHK / CHK) against counting stubs of the few runtime calls the header makes: no HIP
// runtime is linked, nothing runs on a device.  Built with the host compiler under AddressSanitizer and UBSan by tests/test_owned_host.py;
// exit status 0 = every case held (a failed case prints its line and the program exits 1; a leak or a bad free is the sanitizer's to report).
#include "../../convofusion_amd/csrc/owned.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <type_traits>
#include <vector>

// ---- the stubs ----------------------------------------------------------------------------------------
static std::set<void*> g_allocs;          // what hipMalloc handed out and hipFree has not taken back
static int g_mallocs = 0, g_frees = 0, g_bad_frees = 0;
static int g_fail_malloc = 0;             // the next hipMalloc fails
static std::vector<std::string> g_destroyed;   // "exec:<n>" / "graph:<n>" in the order of the destroy calls
static char g_err[512] = "";
static int g_syncs = 0;                   // hipDeviceSynchronize calls
static std::string g_order;               // 'M' malloc, 'S' device synchronise, 'F' free, in call order

extern "C" hipError_t hipMalloc(void** ptr, size_t size) {
  if (g_fail_malloc) {
    g_fail_malloc -= 1;
    *ptr = nullptr;
    return hipErrorOutOfMemory;
  }
  *ptr = malloc(size ? size : 1);
  g_allocs.insert(*ptr);
  g_mallocs += 1;
  g_order += 'M';
  return hipSuccess;
}
extern "C" hipError_t hipFree(void* ptr) {
  if (!g_allocs.erase(ptr)) {
    g_bad_frees += 1;
    return hipErrorInvalidValue;
  }
  free(ptr);
  g_frees += 1;
  g_order += 'F';
  return hipSuccess;
}
extern "C" hipError_t hipDeviceSynchronize(void) {
  g_syncs += 1;
  g_order += 'S';
  return hipSuccess;
}
extern "C" const char* hipGetErrorString(hipError_t) { return "stub error"; }
extern "C" hipError_t hipGraphDestroy(hipGraph_t g) {
  g_destroyed.push_back("graph:" + std::to_string((long long)(size_t)g));
  return hipSuccess;
}
extern "C" hipError_t hipGraphExecDestroy(hipGraphExec_t e) {
  g_destroyed.push_back("exec:" + std::to_string((long long)(size_t)e));
  return hipSuccess;
}
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
std::atomic<long long> g_dbuf_live{0}, g_dbuf_live_bytes{0};

// ---- the cases ----------------------------------------------------------------------------------------
static int g_failed = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
      g_failed += 1;                                                    \
    }                                                                   \
  } while (0)

static_assert(!std::is_copy_constructible<DBuf>::value, "DBuf must not be copyable");
static_assert(!std::is_copy_assignable<DBuf>::value, "DBuf must not be copyable");
static_assert(std::is_nothrow_move_constructible<DBuf>::value && std::is_nothrow_move_assignable<DBuf>::value, "DBuf moves");
static_assert(!std::is_copy_constructible<GraphExec>::value && !std::is_copy_assignable<GraphExec>::value, "GraphExec must not be copyable");
static_assert(std::is_nothrow_move_constructible<GraphExec>::value && std::is_nothrow_move_assignable<GraphExec>::value, "GraphExec moves");

static long long live() { return g_dbuf_live.load(); }
static long long live_bytes() { return g_dbuf_live_bytes.load(); }
// the counters agree with what the stubs have outstanding
static bool consistent() { return live() == (long long)g_allocs.size() && g_bad_frees == 0; }

static void test_ensure() {
  DBuf b;
  EXPECT(b.p == nullptr && b.bytes == 0);
  EXPECT(b.ensure(0) == CFD_OK && b.p == nullptr && g_mallocs == 0);   // nothing asked for: nothing allocated
  EXPECT(b.ensure(100) == CFD_OK && b.p && b.bytes == 100);
  EXPECT(live() == 1 && live_bytes() == 100 && consistent());
  void* first = b.p;
  EXPECT(b.ensure(64) == CFD_OK && b.p == first && b.bytes == 100);    // large enough: kept
  EXPECT(b.ensure(100) == CFD_OK && b.p == first && g_mallocs == 1);
  EXPECT(b.ensure(101) == CFD_OK && b.bytes == 101 && g_mallocs == 2 && g_frees == 1);   // smaller: replaced, the old one freed
  EXPECT(live() == 1 && live_bytes() == 101 && consistent());
  EXPECT(b.as<float>() == reinterpret_cast<float*>(b.p));
  b.release();
  EXPECT(b.p == nullptr && b.bytes == 0 && live() == 0 && live_bytes() == 0 && consistent());
  b.release();                                                         // twice: no second free
  EXPECT(g_bad_frees == 0 && g_frees == 2);
}

static void test_failed_malloc() {
  const int frees = g_frees;
  DBuf b;
  EXPECT(b.ensure(32) == CFD_OK);
  g_fail_malloc = 1;
  g_err[0] = 0;
  EXPECT(b.ensure(64) == CFD_E_HIP);                                   // the old buffer is gone (freed first), no new one came
  EXPECT(b.p == nullptr && b.bytes == 0);
  EXPECT(std::string(g_err).find("hipMalloc") != std::string::npos && std::string(g_err).find("stub error") != std::string::npos);
  EXPECT(g_frees == frees + 1 && live() == 0 && live_bytes() == 0 && consistent());
  EXPECT(b.ensure(16) == CFD_OK && b.bytes == 16 && live() == 1 && live_bytes() == 16);   // usable afterwards
  g_fail_malloc = 1;
  DBuf e;
  EXPECT(e.ensure(8) == CFD_E_HIP && e.p == nullptr && e.bytes == 0 && live() == 1 && consistent());
}

static void test_moves() {
  DBuf a;
  EXPECT(a.ensure(40) == CFD_OK);
  void* pa = a.p;
  DBuf b(std::move(a));                                                // move construction
  EXPECT(a.p == nullptr && a.bytes == 0 && b.p == pa && b.bytes == 40 && live() == 1 && live_bytes() == 40);
  DBuf c;
  c = std::move(b);                                                    // move assignment onto an empty target
  EXPECT(b.p == nullptr && b.bytes == 0 && c.p == pa && c.bytes == 40 && live() == 1);
  DBuf d;
  EXPECT(d.ensure(24) == CFD_OK && live() == 2 && live_bytes() == 64);
  const int frees = g_frees;
  d = std::move(c);                                                    // ... onto a non-empty one: its buffer is freed
  EXPECT(g_frees == frees + 1 && d.p == pa && d.bytes == 40 && c.p == nullptr && live() == 1 && live_bytes() == 40 && consistent());
  DBuf& self = d;
  d = std::move(self);                                                 // self-move keeps the buffer
  EXPECT(d.p == pa && d.bytes == 40 && live() == 1 && consistent());
  a.release();                                                         // a moved-from buffer is empty: nothing to free
  EXPECT(g_bad_frees == 0 && g_frees == frees + 1);
}

struct Layer {                                                         // the LayerW pattern: buffers next to plain pointers
  DBuf w, b;
  const float* g = nullptr;
};
static void test_vector_resize() {
  std::vector<Layer> v;
  v.resize(3);
  for (size_t i = 0; i < v.size(); ++i) {
    EXPECT(v[i].w.ensure(16 * (i + 1)) == CFD_OK && v[i].b.ensure(8) == CFD_OK);
  }
  void* w1 = v[1].w.p;
  EXPECT(live() == 6 && live_bytes() == 16 + 32 + 48 + 24);
  v.resize(40);                                                        // grows past the capacity: the elements move
  EXPECT(v[1].w.p == w1 && v[1].w.bytes == 32 && v[39].w.p == nullptr && live() == 6 && consistent());
  v.resize(1);                                                         // shrinks: the dropped elements free their buffers
  EXPECT(live() == 2 && live_bytes() == 16 + 8 && consistent());
}

static void test_map() {
  std::map<std::string, DBuf> raw;
  DBuf& b = raw["latent_embd.weight"];                                 // default construction in place
  EXPECT(b.p == nullptr && b.ensure(256) == CFD_OK);
  EXPECT(raw["latent_embd.weight"].p == b.p && raw["latent_embd.weight"].ensure(128) == CFD_OK && g_mallocs > 0);
  EXPECT(raw["latent_embd.bias"].ensure(4) == CFD_OK && raw.size() == 2 && live() == 2 && live_bytes() == 260);
  raw.erase("latent_embd.bias");
  EXPECT(live() == 1 && live_bytes() == 256 && consistent());
}

static int later_step(bool ok) { return ok ? CFD_OK : fail(CFD_E_ARG, "refused"); }
static int two_buffers_then(bool ok, bool fail_second) {
  DBuf x, y;
  CHK(x.ensure(1000));
  if (fail_second) g_fail_malloc = 1;
  CHK(y.ensure(2000));
  EXPECT(live() == 2 && live_bytes() == 3000);
  CHK(later_step(ok));                                                 // the early return: both buffers go with the scope
  return CFD_OK;
}
static void test_early_return() {
  EXPECT(two_buffers_then(true, false) == CFD_OK && live() == 0 && consistent());
  EXPECT(two_buffers_then(false, false) == CFD_E_ARG && live() == 0 && live_bytes() == 0 && consistent());
  EXPECT(two_buffers_then(true, true) == CFD_E_HIP && live() == 0 && live_bytes() == 0 && consistent());
}

static hipGraph_t graph_of(size_t n) { return reinterpret_cast<hipGraph_t>(n); }
static hipGraphExec_t exec_of(size_t n) { return reinterpret_cast<hipGraphExec_t>(n); }
struct Keyed {                                                         // the WegState::Graph pattern
  std::vector<long long> key;
  int uses = 0;
  GraphExec gx;
  void reset(const std::vector<long long>& new_key = {}) { *this = Keyed{new_key}; }
};
static void test_graph_exec() {
  typedef std::vector<std::string> Calls;
  {
    GraphExec g;                                                       // null state: nothing to destroy, here or at scope end
    g.reset();
  }
  EXPECT(g_destroyed.empty());
  {
    GraphExec g;
    g.graph = graph_of(1); g.exec = exec_of(2);
    g.reset();                                                         // the executable first, then the graph
    EXPECT((g_destroyed == Calls{"exec:2", "graph:1"}) && g.graph == nullptr && g.exec == nullptr);
    g.graph = graph_of(3);                                             // a capture whose instantiation failed: a graph alone
  }
  EXPECT((g_destroyed == Calls{"exec:2", "graph:1", "graph:3"}));
  g_destroyed.clear();
  {
    GraphExec a;
    a.graph = graph_of(4); a.exec = exec_of(5);
    GraphExec b(std::move(a));
    EXPECT(a.graph == nullptr && a.exec == nullptr && b.graph == graph_of(4) && b.exec == exec_of(5) && g_destroyed.empty());
    GraphExec c;
    c.graph = graph_of(6); c.exec = exec_of(7);
    c = std::move(b);                                                  // onto a non-empty target: its graph is destroyed
    EXPECT((g_destroyed == Calls{"exec:7", "graph:6"}) && b.graph == nullptr && b.exec == nullptr && c.exec == exec_of(5));
    a.reset(); b.reset();                                              // moved-from: nothing
    EXPECT(g_destroyed.size() == 2);
  }
  EXPECT((g_destroyed == Calls{"exec:7", "graph:6", "exec:5", "graph:4"}));   // each pair once
  g_destroyed.clear();
  {
    Keyed k;
    k.key = {1, 2}; k.uses = 3;
    k.gx.graph = graph_of(8); k.gx.exec = exec_of(9);
    k.reset({7});
    EXPECT((g_destroyed == Calls{"exec:9", "graph:8"}) && k.key == std::vector<long long>{7} && k.uses == 0 && k.gx.exec == nullptr);
    k.reset();
    EXPECT(g_destroyed.size() == 2 && k.key.empty());
  }
  EXPECT(g_destroyed.size() == 2);
}

// ArenaLayout: one statement of a workspace's buffers, run to size (null base) and run to carve.  Three field lists whose counts are no
// multiples of the granule, at the granules the library uses (4 floats: the VAE decode; 64: the row-tile arenas).
struct Fields {                                                        // buffers of more than one element type, like RtSave
  float* f[6];
  char* bytes;
  int* ints;
};
static void test_arena_layout() {
  const std::vector<std::vector<size_t>> lists = {{1, 2, 3, 5, 7, 9, 11, 13}, {63, 65, 127, 129, 1, 4097, 640, 3}, {1000003, 1, 0, 17, 255, 257, 5, 64}};
  for (size_t granule : {(size_t)4, (size_t)64}) {
    for (const std::vector<size_t>& n : lists) {
      Fields fd;
      auto layout = [&](ArenaLayout a) {                               // each buffer named once, in the order it is carved
        for (int k = 0; k < 6; ++k) a.take(fd.f[k], n[k]);
        a.take(fd.bytes, n[6]);
        a.take(fd.ints, n[7]);
        return a.bytes();
      };
      const size_t need = layout(ArenaLayout(nullptr, granule));
      EXPECT(fd.f[0] == nullptr && fd.bytes == nullptr && fd.ints == nullptr);   // the sizing pass hands out nothing
      size_t sum = 0;
      for (size_t v : n) sum += (v + granule - 1) / granule * granule;
      EXPECT(need == sum * sizeof(float));                             // every count rounded up to the granule, nothing else
      std::vector<float> mem(need / sizeof(float) + 1, 0.f);          // (+ 1: an address one past the arena stays a valid one)
      EXPECT(layout(ArenaLayout(mem.data(), granule)) == need);        // the carving pass consumes exactly what the sizing pass asked for
      const float* at[9] = {fd.f[0], fd.f[1], fd.f[2], fd.f[3], fd.f[4], fd.f[5], reinterpret_cast<float*>(fd.bytes),
                            reinterpret_cast<float*>(fd.ints), mem.data() + need / sizeof(float)};
      EXPECT(at[0] == mem.data());
      for (int k = 0; k < 8; ++k) {
        EXPECT((size_t)(at[k] - mem.data()) % granule == 0);           // granule-aligned,
        EXPECT(at[k + 1] >= at[k] + n[k]);                             // in call order, and disjoint: buffer k ends before k + 1 starts
        EXPECT((size_t)(at[k + 1] - at[k]) < n[k] + granule);          // ... with less than one granule between them
      }
      for (int k = 0; k < 6; ++k)
        for (size_t i = 0; i < n[k]; ++i) fd.f[k][i] = (float)(k + 1); // (under AddressSanitizer: every element lies inside the allocation)
      for (int k = 0; k < 6; ++k) EXPECT(n[k] == 0 || (fd.f[k][0] == (float)(k + 1) && fd.f[k][n[k] - 1] == (float)(k + 1)));
    }
  }
  ArenaLayout y(nullptr, 64);
  EXPECT(y.rounded(0) == 0 && y.rounded(1) == 64 && y.rounded(64) == 64 && y.rounded(65) == 128 && y.bytes() == 0);
  if (!g_failed) printf("ArenaLayout: %d layouts sized and carved alike\n", (int)(2 * lists.size()));
}

// carve and DBuf::grow: one layout sized, grown by the one rule -- the device is waited for before a block that holds memory is freed,
// and only then -- and carved; at both granules.
struct Ws {
  float *a, *b, *none;
  int* ints;
  float* c;
};
static void ws_layout(ArenaLayout& y, Ws& w, size_t n) {               // counts that are multiples of neither granule; `none` has no floats
  y.take(w.a, n + 1); y.take(w.b, 3 * n + 2); y.take(w.none, 0); y.take(w.ints, n + 5); y.take(w.c, 7);
}
static bool ws_same(const Ws& x, const Ws& y) { return x.a == y.a && x.b == y.b && x.none == y.none && x.ints == y.ints && x.c == y.c; }
static Ws ws_by_hand(const DBuf& ws, size_t granule, size_t n, size_t* bytes) {
  Ws w{};
  ArenaLayout y(ws.as<float>(), granule);
  ws_layout(y, w, n);
  *bytes = y.bytes();
  return w;
}
static void test_carve() {
  int cases = 0;
  for (size_t granule : {(size_t)4, (size_t)64}) {
    DBuf ws;
    Ws w{};
    bool grew = false;
    size_t need = 0;
    auto carve_n = [&](size_t n) { return carve(ws, granule, [&](ArenaLayout& y) { ws_layout(y, w, n); }, &grew); };
    int m = g_mallocs, f = g_frees, s = g_syncs;
    EXPECT(carve_n(10) == CFD_OK && grew);                             // an empty buffer: one allocation, nothing to wait for
    EXPECT(g_mallocs == m + 1 && g_frees == f && g_syncs == s && live() == 1 && consistent());
    const Ws first = ws_by_hand(ws, granule, 10, &need);               // every field is what a hand-run ArenaLayout gives
    EXPECT(ws_same(w, first) && ws.bytes == need && live_bytes() == (long long)need && w.a == ws.as<float>());
    EXPECT(w.none != nullptr && w.none == reinterpret_cast<float*>(w.ints));   // no floats, still an address: the next buffer's
    for (size_t i = 0; i < 11; ++i) w.a[i] = 1.f;                      // (under AddressSanitizer: the ends lie inside the allocation)
    for (size_t i = 0; i < 7; ++i) w.c[i] = 2.f;
    EXPECT(w.c + 7 <= ws.as<float>() + need / sizeof(float));
    void* base = ws.p;
    EXPECT(carve_n(10) == CFD_OK && !grew);                            // the same layout again: nothing allocated, nothing waited for
    EXPECT(g_mallocs == m + 1 && g_frees == f && g_syncs == s && ws.p == base && ws_same(w, first));
    g_order.clear();
    EXPECT(carve_n(100) == CFD_OK && grew);                            // a larger one: exactly one wait, before the free
    EXPECT(g_order == "SFM" && g_syncs == s + 1 && live() == 1 && consistent());
    const Ws big = ws_by_hand(ws, granule, 100, &need);
    EXPECT(ws_same(w, big) && ws.bytes == need && live_bytes() == (long long)need);
    base = ws.p;
    m = g_mallocs, f = g_frees, s = g_syncs;
    size_t small = 0;
    EXPECT(carve_n(10) == CFD_OK && !grew);                            // a smaller one afterwards: the allocation stays as it is
    EXPECT(g_mallocs == m && g_frees == f && g_syncs == s && ws.p == base && ws.bytes == need);
    EXPECT(ws_same(w, ws_by_hand(ws, granule, 10, &small)) && small < need);
    g_fail_malloc = 1;
    g_order.clear();
    g_err[0] = 0;
    EXPECT(carve_n(1000) == CFD_E_HIP && grew);                        // hipMalloc fails: the error comes back, the buffer is empty
    EXPECT(std::string(g_err).find("hipMalloc") != std::string::npos && g_order == "SF");
    EXPECT(ws.p == nullptr && ws.bytes == 0 && live() == 0 && live_bytes() == 0 && consistent());
    EXPECT(w.a == nullptr && w.none == nullptr && w.c == nullptr);     // ... and no field points into the block that was freed
    s = g_syncs;
    EXPECT(carve_n(10) == CFD_OK && grew && g_syncs == s && live() == 1);   // usable afterwards; empty again, so no wait
    cases += 1;
  }
  DBuf d;                                                              // the primitive alone (one buffer, no layout)
  bool grew = true;
  const int s = g_syncs;
  EXPECT(d.grow(0, &grew) == CFD_OK && !grew && d.p == nullptr);
  EXPECT(d.grow(32, &grew) == CFD_OK && grew && d.bytes == 32 && g_syncs == s);
  EXPECT(d.grow(16, &grew) == CFD_OK && !grew && d.bytes == 32 && g_syncs == s);
  g_order.clear();
  EXPECT(d.grow(64) == CFD_OK && d.bytes == 64 && g_order == "SFM" && consistent());
  if (!g_failed) printf("carve: %d granules grown by one rule, the wait before the free\n", cases);
}

int main() {
  test_arena_layout();
  test_ensure();
  test_failed_malloc();
  EXPECT(live() == 0 && live_bytes() == 0 && consistent());
  test_carve();
  EXPECT(live() == 0 && live_bytes() == 0 && consistent());
  test_moves();
  EXPECT(live() == 0 && live_bytes() == 0 && consistent());
  test_vector_resize();
  test_map();
  test_early_return();
  test_graph_exec();
  EXPECT(live() == 0 && live_bytes() == 0);                            // the live counters are 0 at the end ...
  EXPECT(g_allocs.empty() && g_mallocs == g_frees && g_bad_frees == 0);   // ... and so is what the stubs have outstanding
  if (g_failed) {
    printf("%d checks FAILED\n", g_failed);
    return 1;
  }
  printf("owned.hpp: all checks passed (%d allocations, %d frees)\n", g_mallocs, g_frees);
  return 0;
}
