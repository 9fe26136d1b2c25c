// cfd_weg_eval on the row-tile gradient engine (rt_grad.hpp, compiled in cfd_grad.hip): the product path of the word-excitation-guidance
// evaluation for small problems (the reference needs test batch size 1 for WEG, word_excitation_guidance.py:25).
// ~160 launches of ~5 us instead of weg_eval.hpp's ~400 launches of ~10 us, in the folded formulation the sampling loop itself uses.
// WEG's own part: the forward stops behind the top layer's cross-attention, the objective and its gradient at the nine text maps follow
// (the focus kernels of grad.hpp), and the sweep starts from them.
// Included by cfd_weg.hip after weg_eval.hpp.
#pragma once

namespace wegrt {

static bool eligible(Ctx* c, const cfd_weg_args* a) { return !rtgrad::ineligible(c, a->B, a->L, a->mem); }

// forward with saved activations, then the objective and its gradient at the nine maps
static int enqueue_forward_and_objective(Ctx* c, hipStream_t st, const weg::Args& e) {
  RtGradState& s = c->grad.rt;
  const int nl = c->nl, B = s.B, L = s.L, St = s.St;
  CHK(rtgrad::enqueue_forward_saved(c, st, e.latents));
  s.focus_large = !(L * (e.last - 1) <= WEG_SMALL_CELLS && e.nt_max <= WEG_SMALL_TOK && L <= 64);
  if (!s.focus_large)
    hipLaunchKernelGGL(weg_focus_small_kernel<>, dim3((unsigned)B), dim3(256), 0, st, s.att, e.tok_off, e.tok_idx, B, nl, L, St, e.last, e.k3[0], e.k3[1],
                       e.k3[2], e.losses, e.max_att, s.d_att);
  else
    hipLaunchKernelGGL(weg_focus_kernel<>, dim3((unsigned)B), dim3(256), 0, st, s.att, e.tok_off, e.tok_idx, B, nl, L, St, e.last, e.nt_max, e.k3[0], e.k3[1],
                       e.k3[2], s.fws, e.losses, e.max_att, s.d_att);
  HIPCHK(hipGetLastError());
  ++s.launches;
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

}  // namespace wegrt
