// libcfdenoise: the resources that free themselves -- a device buffer (DBuf), a captured graph with its executable (GraphExec) --, the layout of
// a workspace carved into buffers (ArenaLayout) and the one way a call sizes, grows and carves its workspace (carve), and the error helpers
// they return through.  Host code only, no kernel header: tests/host/owned_test.cpp builds it against stubs of the runtime calls it makes.
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <utility>

#include "../../include/cfdenoise.h"

int fail(int code, const char* fmt, ...);      // cfd_core.hip: formats the thread's last-error text (cfd_last_error) and returns `code`
#define HIPCHK(expr)                                                                               \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) return fail(CFD_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)
#define CHK(expr)            \
  do {                       \
    int _r = (expr);         \
    if (_r != CFD_OK) return _r; \
  } while (0)

// The process's DBufs that hold memory, and their bytes (cfd_core.hip; read-out: cfd_debug_live_buffers)
extern std::atomic<long long> g_dbuf_live, g_dbuf_live_bytes;

// A device allocation and its owner: freed by the destructor, handed on by a move (which leaves the source empty), never copied.  hipFree waits
// for the device, so no DBuf goes out of scope in a per-step path: they live on the handle, in a workspace, or in set-up code and developer hooks.
struct DBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DBuf() = default;
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  DBuf(DBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
  DBuf& operator=(DBuf&& o) noexcept { if (this != &o) { release(); p = std::exchange(o.p, nullptr); bytes = std::exchange(o.bytes, 0); } return *this; }
  ~DBuf() { release(); }
  int ensure(size_t n) {        // at least n bytes; a buffer that has to grow loses its contents
    if (n <= bytes) return CFD_OK;
    release();
    HIPCHK(hipMalloc(&p, n));
    bytes = n;
    g_dbuf_live += 1; g_dbuf_live_bytes += (long long)n;
    return CFD_OK;
  }
  // The growth rule of a workspace that launches of earlier calls, on any stream, may still read: at least n bytes, and the device is
  // waited for before a block that holds memory is released (an empty buffer has nothing to wait for).  *grew: it had to grow.
  // A workspace that is large enough costs a comparison.  Host work that waits: never under a stream capture.
  int grow(size_t n, bool* grew = nullptr) {
    if (grew) *grew = n > bytes;
    if (n <= bytes) return CFD_OK;
    if (p) HIPCHK(hipDeviceSynchronize());
    return ensure(n);
  }
  void release() {              // (the destructor does this: called only where a buffer is freed early on purpose)
    if (p) { (void)hipFree(p); g_dbuf_live -= 1; g_dbuf_live_bytes -= (long long)bytes; }
    p = nullptr; bytes = 0;
  }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// The layout of a workspace of floats, stated once and run twice (carve, below): with a null base it sizes (bytes() is what to
// allocate), with the allocation as base it carves the same buffers in the same order.  Each buffer is named once -- take(field, count)
// -- and occupies its count rounded up to `granule` floats; a buffer of 0 floats still gets the (non-null) address of the next one.
struct ArenaLayout {
  float* base;                  // null: the sizing pass, which leaves every field null
  size_t granule, off = 0;      // floats
  ArenaLayout(float* base_, size_t granule_) : base(base_), granule(granule_) {}
  size_t rounded(size_t count) const { return (count + granule - 1) / granule * granule; }
  template <class T> void take(T*& field, size_t count) {
    field = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += rounded(count);
  }
  size_t bytes() const { return off * sizeof(float); }
};

// A call's workspace: `layout` names every buffer once (take, in carving order); it runs with a null base to size, `ws` grows by
// DBuf::grow's rule, and it runs again over the allocation.  A failed allocation leaves `ws` empty and every field null.
template <class Layout>
int carve(DBuf& ws, size_t granule, Layout&& layout, bool* grew = nullptr) {
  ArenaLayout size(nullptr, granule);
  layout(size);
  CHK(ws.grow(size.bytes(), grew));
  ArenaLayout lay(ws.as<float>(), granule);
  layout(lay);
  return CFD_OK;
}

// A captured graph and its executable, destroyed together (executable first); move-only like DBuf.
struct GraphExec {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  GraphExec() = default;
  GraphExec(const GraphExec&) = delete;
  GraphExec& operator=(const GraphExec&) = delete;
  GraphExec(GraphExec&& o) noexcept : graph(std::exchange(o.graph, nullptr)), exec(std::exchange(o.exec, nullptr)) {}
  GraphExec& operator=(GraphExec&& o) noexcept { if (this != &o) { reset(); graph = std::exchange(o.graph, nullptr); exec = std::exchange(o.exec, nullptr); } return *this; }
  ~GraphExec() { reset(); }
  void reset() {
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    exec = nullptr; graph = nullptr;
  }
};
