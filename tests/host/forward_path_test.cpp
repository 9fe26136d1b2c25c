// Host test of csrc/forward_path.hpp: decide_forward_path over a table of inputs, every field of the result checked.  One case per arm
// the library distinguishes.  The expected values were read off the conditions as they stood where they used to be written -- setup_problem,
// prepare_static_memside, build_xattn_worklist's length gate, enqueue_rows, wire_att_ring and operand_policy_and_census -- not taken from
// the function.  Built with the host compiler under AddressSanitizer and UBSan by tests/test_forward_path_host.py; exit status 0 = every
// case held (a failed case prints its fields and the program exits 1).
#include "../../convofusion_amd/csrc/forward_path.hpp"

#include <cstdio>
#include <functional>
#include <vector>

struct Case {
  const char* name;
  PathKnobs k;
  PathShape s;
  PathAsk a;
  ForwardPath want;
};

static const int ALL = 31;

// B = 2 utterances x G = 7 chunks of 16 tokens, memories of (6, 20, 6, 8, 1) keys: 224 token rows, 160 padded keys, 4 workgroups of 4 query tiles
static PathShape shape(int Be = 14, int L = 16, int tmode = 0, int audio = 20) {
  PathShape s;
  s.Be = Be; s.L = L; s.tmode = tmode;
  const int S[FP_NMEM] = {6, audio, 6, 8, 1};
  for (int j = 0; j < FP_NMEM; ++j) s.S[j] = S[j];
  return s;
}
// the tile kernels with the length gate lifted (CFD_ROWTILE=0 CFD_FUSED_XATTN_MIN_WGS=0), then one more change
static PathKnobs tile(const std::function<void(PathKnobs&)>& more = nullptr) {
  PathKnobs k;
  k.rt_on = false; k.min_wgs = 0;
  if (more) more(k);
  return k;
}
static PathAsk ask(const std::function<void(PathAsk&)>& more = nullptr) {
  PathAsk a;
  if (more) more(a);
  return a;
}
static ForwardPath want(bool rt, int xattn, int inst, bool list, int f16_mask, int share_rows, bool ln_fold, bool rows_now, int static_mask) {
  ForwardPath p;
  p.rt = rt; p.xattn = xattn; p.xa_inst = inst; p.xa_list = list; p.f16_mask = f16_mask; p.share = share_rows > 0; p.share_rows = share_rows;
  p.ln_fold = ln_fold; p.rows_now = rows_now; p.dstep_slot = rows_now ? 0 : 1; p.static_mask = static_mask;
  return p;
}

static ForwardPath unreached(ForwardPath p) {
  p.xa_reached = false;
  return p;
}

int main() {
  const PathKnobs dflt;
  const auto chunks2 = [](PathAsk& a) { a.chunk_rows = 2; };
  const auto f16 = [](PathAsk& a) { a.f16 = true; };
  const auto ring = [](PathAsk& a) { a.ring_row0 = 12; a.ring_rows = 2; };
  const auto att = [](PathAsk& a) { a.att_out = true; };
  const std::vector<Case> cases = {
    // ---- the forward: row-tile by shape, and what loses it
    {"row-tile by shape (default gate: 4 workgroups < 6, no list)", dflt, shape(), ask(chunks2),
     want(true, XATTN_ROWTILE, XA_INST_NONE, false, 0, 0, false, true, ALL)},
    {"CFD_ROWTILE=0", tile(), shape(), ask(chunks2), want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 2, false, true, ALL)},
    {"too many rows (704 > 700; 11 workgroups pass the default gate; the fold's range)", dflt, shape(44), ask(),
     want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, true, true, ALL)},
    {"700 rows exactly stay (L = 28)", dflt, shape(25, 28), ask(), want(true, XATTN_ROWTILE, XA_INST_NONE, true, 0, 0, false, true, ALL)},
    {"L = 34 > RT_MAX_L (2 workgroups: three-launch)", dflt, shape(2, 34), ask(), want(false, XATTN_THREE, XA_INST_NONE, false, 0, 0, false, true, 0)},
    {"too many keys (1152 padded > RT_MAX_KEYS)", tile([](PathKnobs& k) { k.rt_on = true; }), shape(14, 16, 0, 1000), ask(),
     want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, false, true, ALL)},
    {"1024 padded keys exactly stay", dflt, shape(14, 16, 0, 890), ask(), want(true, XATTN_ROWTILE, XA_INST_NONE, false, 0, 0, false, true, ALL)},
    {"per-row timesteps: fused kernel on per-call projections, step index read by the launches", tile([](PathKnobs& k) { k.rt_on = true; }),
     shape(14, 16, 1), ask(), want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, false, false, 0)},
    {"a level batch", tile([](PathKnobs& k) { k.rt_on = true; }), shape(28, 16, 2), ask(),
     want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, false, false, 0)},
    {"a dynamic memory leaves the row-tile path; the others stay static", tile([](PathKnobs& k) { k.rt_on = true; }), shape(),
     ask([](PathAsk& a) { a.dynamic_mask = 16; a.chunk_rows = 2; }), want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 2, false, true, 15)},
    // ---- fused kernel against three-launch
    {"CFD_FUSED_XATTN=0 (the head is still shared)", tile([](PathKnobs& k) { k.fused_xattn = false; }), shape(), ask(chunks2),
     want(false, XATTN_THREE, XA_INST_NONE, false, 0, 2, false, true, 0)},
    {"length gate 6: 5 workgroups", tile([](PathKnobs& k) { k.min_wgs = 6; }), shape(20), ask(),
     want(false, XATTN_THREE, XA_INST_NONE, false, 0, 0, false, true, 0)},
    {"length gate 6: 6 workgroups", tile([](PathKnobs& k) { k.min_wgs = 6; }), shape(21), ask(),
     want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, false, true, ALL)},
    {"length gate 0: one workgroup", tile(), shape(1, 2), ask(), want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, false, true, ALL)},
    {"attention outputs, ATT instance available", tile(), shape(), ask(att), want(false, XATTN_FUSED, XA_INST_ATT, true, 0, 0, false, true, ALL)},
    {"attention outputs, no fused kernel: three-launch", tile([](PathKnobs& k) { k.fused_xattn = false; }), shape(), ask(att),
     want(false, XATTN_THREE, XA_INST_NONE, false, 0, 0, false, true, 0)},
    {"attention outputs below the gate: three-launch", tile([](PathKnobs& k) { k.min_wgs = 6; }), shape(), ask(att),
     want(false, XATTN_THREE, XA_INST_NONE, false, 0, 0, false, true, 0)},
    {"attention outputs with per-row timesteps: three-launch (the list is built, unused)", tile(), shape(14, 16, 1), ask(att),
     want(false, XATTN_THREE, XA_INST_NONE, true, 0, 0, false, false, 0)},
    {"attention outputs on the row-tile path", dflt, shape(), ask(att), want(true, XATTN_ROWTILE, XA_INST_NONE, false, 0, 0, false, true, ALL)},
    {"dynamic memories keep the fused kernel", tile(), shape(), ask([](PathAsk& a) { a.dynamic_mask = 5; }),
     want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, false, true, 26)},
    // ---- the three instances
    {"attention ring on the tile kernels: ATT", tile(), shape(), ask(ring), want(false, XATTN_FUSED, XA_INST_ATT, true, 0, 0, false, true, ALL)},
    {"attention ring on the row-tile path", dflt, shape(), ask(ring), want(true, XATTN_ROWTILE, XA_INST_NONE, false, 0, 0, false, true, ALL)},
    {"attention ring with a dynamic memory: no kernel keeps the maps (wire_att_ring refuses the run)", tile(), shape(),
     ask([](PathAsk& a) { a.ring_row0 = 12; a.ring_rows = 2; a.dynamic_mask = 1; }), want(false, XATTN_THREE, XA_INST_NONE, true, 0, 0, false, true, 0)},
    {"F16: a 128-key memory, all static, no maps, tile kernels, one timestep", tile(), shape(14, 16, 0, 100), ask(f16),
     want(false, XATTN_FUSED, XA_INST_F16, true, 2, 0, false, true, ALL)},
    {"F16 asked, 96 padded keys: pairs", tile(), shape(14, 16, 0, 96), ask(f16), want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, false, true, ALL)},
    {"F16 asked, a dynamic memory: pairs", tile(), shape(14, 16, 0, 100), ask([](PathAsk& a) { a.f16 = true; a.dynamic_mask = 16; }),
     want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, false, true, 15)},
    {"F16 asked, maps kept: ATT", tile(), shape(14, 16, 0, 100), ask([](PathAsk& a) { a.f16 = true; a.ring_row0 = 12; a.ring_rows = 2; }),
     want(false, XATTN_FUSED, XA_INST_ATT, true, 0, 0, false, true, ALL)},
    {"F16 asked on the row-tile path", tile([](PathKnobs& k) { k.rt_on = true; }), shape(14, 16, 0, 100), ask(f16),
     want(true, XATTN_ROWTILE, XA_INST_NONE, true, 0, 0, false, true, ALL)},
    {"F16 asked with per-row timesteps: pairs", tile(), shape(14, 16, 1, 100), ask(f16), want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, false, false, 0)},
    {"F16 asked, three-launch", tile([](PathKnobs& k) { k.min_wgs = 6; }), shape(14, 16, 0, 100), ask(f16),
     want(false, XATTN_THREE, XA_INST_NONE, false, 0, 0, false, true, 0)},
    // ---- share
    {"share: G = 1", tile(), shape(2), ask(chunks2), want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, false, true, ALL)},
    {"share: CFD_SHARE0=0", tile([](PathKnobs& k) { k.share0 = false; }), shape(), ask(chunks2),
     want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, false, true, ALL)},
    {"share: Be = 15 is no multiple of 2", tile(), shape(15), ask(chunks2), want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, false, true, ALL)},
    {"share: off under stop_stage (4: behind layer 0's cross-attention)", tile([](PathKnobs& k) { k.stop_stage = 4; }), shape(), ask(chunks2),
     want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, false, true, ALL)},
    {"stop_stage 3 ends the forward in front of the first cross-attention: the instance is decided, none is reached", tile([](PathKnobs& k) { k.stop_stage = 3; }),
     shape(), ask(att), unreached(want(false, XATTN_FUSED, XA_INST_ATT, true, 0, 0, false, true, ALL))},
    // ---- ln_fold (L = 16: M is a multiple of 16, so 496 / 512 and 3840 / 3856 are the rows on either side of the range's ends)
    {"ln_fold forced on", tile([](PathKnobs& k) { k.ln_fold = 1; }), shape(), ask(), want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, true, true, ALL)},
    {"ln_fold forced off", tile([](PathKnobs& k) { k.ln_fold = 0; }), shape(44), ask(), want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, false, true, ALL)},
    {"ln_fold by shape: M = 496", tile(), shape(31), ask(), want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, false, true, ALL)},
    {"ln_fold by shape: M = 512", tile(), shape(32), ask(), want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, true, true, ALL)},
    {"ln_fold by shape: M = 3840", tile(), shape(240), ask(), want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, true, true, ALL)},
    {"ln_fold by shape: M = 3856", tile(), shape(241), ask(), want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, false, true, ALL)},
    {"ln_fold: L = 18, M = 576", tile(), shape(32, 18), ask(), want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, false, true, ALL)},
    {"ln_fold forced on, L = 18", tile([](PathKnobs& k) { k.ln_fold = 1; }), shape(32, 18), ask(),
     want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, false, true, ALL)},
    {"ln_fold: off under stop_stage", tile([](PathKnobs& k) { k.stop_stage = 7; }), shape(44), ask(),
     want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, false, true, ALL)},
    {"ln_fold forced on: off under stop_stage", tile([](PathKnobs& k) { k.stop_stage = 37; k.ln_fold = 1; }), shape(44), ask(),
     want(false, XATTN_FUSED, XA_INST_PAIR, true, 0, 0, false, true, ALL)},
  };
  int bad = 0;
  for (const Case& c : cases) {
    const ForwardPath g = decide_forward_path(c.k, c.s, c.a), &w = c.want;
    const bool ok = g.rt == w.rt && g.xattn == w.xattn && g.xa_inst == w.xa_inst && g.xa_list == w.xa_list && g.f16_mask == w.f16_mask &&
                    g.share == w.share && g.share_rows == w.share_rows && g.ln_fold == w.ln_fold && g.rows_now == w.rows_now &&
                    g.dstep_slot == w.dstep_slot && g.static_mask == w.static_mask && g.xa_reached == w.xa_reached && g.keeps_maps() == (w.xa_inst == XA_INST_ATT);
    if (ok) continue;
    bad += 1;
    const ForwardPath* both[2] = {&g, &w};
    for (int i = 0; i < 2; ++i) {
      const ForwardPath& p = *both[i];
      printf("%s %s: rt=%d xattn=%d xa_inst=%d xa_reached=%d xa_list=%d f16_mask=%d share=%d share_rows=%d ln_fold=%d rows_now=%d dstep_slot=%d static_mask=%d\n",
             i ? "  want" : "FAILED", i ? "" : c.name, p.rt, p.xattn, p.xa_inst, p.xa_reached, p.xa_list, p.f16_mask, p.share, p.share_rows, p.ln_fold, p.rows_now,
             p.dstep_slot, p.static_mask);
    }
  }
  if (bad) {
    printf("%d of %zu cases failed\n", bad, cases.size());
    return 1;
  }
  printf("%zu cases: all checks passed\n", cases.size());
  return 0;
}
