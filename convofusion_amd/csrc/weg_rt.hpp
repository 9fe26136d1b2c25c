// cfd_weg_eval on the row-tile gradient engine (rt_grad.hpp, compiled in cfd_grad.hip): the product path of the word-excitation-guidance
// evaluation for small problems (the reference needs test batch size 1 for WEG, word_excitation_guidance.py:25).
// ~160 launches of ~5 us instead of weg_eval.hpp's ~400 launches of ~10 us, in the folded formulation the sampling loop itself uses.
// WEG's own part: the forward stops behind the top layer's cross-attention, the objective and its gradient at the nine text maps follow
// (the focus kernels of grad.hpp), and the sweep starts from them.
// cfd_weg_step runs on the same engine with every row its own utterance (weg::Args::last_rows) and ends in weg_rows_update_kernel: the
// per-row gated update, with the fold of tied tokens' gradients onto their sources.
// Included by cfd_weg.hip after weg_eval.hpp.
#pragma once

struct WegRowsUpdateArgs {
  const float* x;        // [n_tok][128]: x~ (with a tie never the caller's latents: x_new may alias those)
  const float* g;        // [n_tok][128]: g~, the sweep's gradient of every row's own loss at x~
  const float* step;     // [n_tok / L]: the rows' steps, or null (every step 0)
  const int32_t* tie;    // [n_tok] or null
  const int32_t* csr;    // guide_tables.hpp, or null
  float* grad;           // [n_tok][128] or null
  float* x_new;          // [n_tok][128] or null
  long long n_tok;
  int L;
};

// One thread per float4 of [n_tok][128].  A free token s in row r(s) = s / L, with T(s) the tokens tied to s in ascending order (the CSR
// table):
//   grad[s]  = g~[s] + sum_{t in T(s)} g~[t]                               (folded, unstepped)
//   x_new[s] = x~[s] - (step[r(s)] g~[s] + sum_{t in T(s)} step[r(t)] g~[t])
// -- a tied token's gradient serves the loss of the row it sits in, so it is weighted by that row's step.  A tied token runs its SOURCE's
// instructions, so it takes the source's new value bit for bit; its own gradient is 0.  No atomics: the same bits every time.  Table
// entries out of range are skipped (guide_update_kernel's rule): no table reads out of bounds.
template <int = 0>
__global__ void weg_rows_update_kernel(WegRowsUpdateArgs a) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= a.n_tok * 32) return;
  const long long tok = i >> 5;
  const int q = (int)(i & 31);
  const int v = a.tie ? a.tie[tok] : -1;
  const bool tied = v >= 0 && v < a.n_tok;
  const long long s = tied ? v : tok;
  float4 gu = reinterpret_cast<const float4*>(a.g)[s * 32 + q];
  const float st = a.step ? a.step[s / a.L] : 0.f;
  float4 gs = make_float4(st * gu.x, st * gu.y, st * gu.z, st * gu.w);
  if (a.csr) {
    const long long lo = a.csr[s], hi = a.csr[s + 1];
    const long long beg = lo < 0 ? 0 : (lo > a.n_tok ? a.n_tok : lo), end = hi < beg ? beg : (hi > a.n_tok ? a.n_tok : hi);
    for (long long k = beg; k < end; ++k) {
      const int t = a.csr[a.n_tok + 1 + k];
      if (t < 0 || t >= a.n_tok) continue;
      const float4 r = reinterpret_cast<const float4*>(a.g)[(long long)t * 32 + q];
      const float sr = a.step ? a.step[t / a.L] : 0.f;
      gu.x += r.x; gu.y += r.y; gu.z += r.z; gu.w += r.w;
      gs.x += sr * r.x; gs.y += sr * r.y; gs.z += sr * r.z; gs.w += sr * r.w;
    }
  }
  if (a.x_new) {
    const float4 x = reinterpret_cast<const float4*>(a.x)[s * 32 + q];
    reinterpret_cast<float4*>(a.x_new)[i] = make_float4(x.x - gs.x, x.y - gs.y, x.z - gs.z, x.w - gs.w);
  }
  if (a.grad) reinterpret_cast<float4*>(a.grad)[i] = tied ? make_float4(0.f, 0.f, 0.f, 0.f) : gu;
}

namespace wegrt {

static bool eligible(Ctx* c, const cfd_weg_args* a) { return !rtgrad::ineligible(c, a->B, a->L, a->mem); }

// Which focus kernel a problem takes: the small one while the maps of the widest slice, the focus tokens and the frames fit its LDS.
static bool focus_small(int L, int last, int nt_max) { return L * (last - 1) <= WEG_SMALL_CELLS && nt_max <= WEG_SMALL_TOK && L <= 64; }

// forward with saved activations, then the objective and its gradient at the nine maps
static int enqueue_forward_and_objective(Ctx* c, hipStream_t st, const weg::Args& e) {
  RtGradState& s = c->grad.rt;
  const int nl = c->nl, B = s.B, L = s.L, St = s.St;
  const int grad_rows = e.last_rows ? 1 : B;
  CHK(rtgrad::enqueue_forward_saved(c, st, e.latents));
  s.focus_large = !focus_small(L, e.last, e.nt_max);
  if (!s.focus_large)
    LAUNCH_COUNTED(s.launches, weg_focus_small_kernel<>, dim3((unsigned)B), dim3(256), 0, st, s.att, e.tok_off, e.tok_idx, B, nl, L, St, e.last, e.k3[0], e.k3[1],
                   e.k3[2], e.losses, e.max_att, s.d_att, e.last_rows, grad_rows);
  else
    LAUNCH_COUNTED(s.launches, weg_focus_kernel<>, dim3((unsigned)B), dim3(256), 0, st, s.att, e.tok_off, e.tok_idx, B, nl, L, St, e.last, e.nt_max, e.k3[0], e.k3[1],
                   e.k3[2], s.fws, e.losses, e.max_att, s.d_att, e.last_rows, grad_rows);
  return CFD_OK;
}

// Launches only (capturable): [time tables + memory side when `full`], forward and objective, reverse sweep.
static int enqueue(Ctx* c, hipStream_t st, bool full, const weg::Args& e) {
  rtgrad::WorkGuard guard(c);
  rtgrad::begin_sequence(c);
  if (full) CHK(rtgrad::enqueue_memory_side(c, st));
  CHK(enqueue_forward_and_objective(c, st, e));
  return rtgrad::enqueue_reverse_sweep(c, st, rtgrad::SweepSeed{}, e.grad);
}

// cfd_weg_step's launches: x~ (with a tie), [time tables + memory side when `full`], the forward with saves from x~ and the per-row
// objective, the reverse sweep into e.grad (= g~), the gated update.  e.latents: the caller's latents; xin: room for x~.
static int enqueue_step(Ctx* c, hipStream_t st, bool full, weg::Args e, float* xin, const float* step, const int32_t* tie, const int32_t* csr,
                        float* grad, float* x_new) {
  rtgrad::WorkGuard guard(c);
  rtgrad::begin_sequence(c);
  RtGradState& s = c->grad.rt;
  const long long n_tok = (long long)s.B * s.L, total4 = n_tok * (CFD_LAT / 4);
  const dim3 grid((unsigned)((total4 + 255) / 256));
  if (tie) {
    LAUNCH_COUNTED(s.launches, guide_replicate_kernel<>, grid, dim3(256), 0, st, e.latents, tie, xin, n_tok, total4);
    e.latents = xin;
  }
  if (full) CHK(rtgrad::enqueue_memory_side(c, st));
  CHK(enqueue_forward_and_objective(c, st, e));
  CHK(rtgrad::enqueue_reverse_sweep(c, st, rtgrad::SweepSeed{}, e.grad));
  if (grad || x_new) {
    WegRowsUpdateArgs ua{e.latents, e.grad, step, tie, tie ? csr : nullptr, grad, x_new, n_tok, s.L};
    LAUNCH_COUNTED(s.launches, weg_rows_update_kernel<>, grid, dim3(256), 0, st, ua);
  }
  return CFD_OK;
}

}  // namespace wegrt
