"""CPU: the Python drivers of an open sampling run -- ``sampler.sample``, ``sample_with_weg``, ``sample_with_loss_guidance`` -- as the
sequence of calls they make on the run and on ``last_step_attention``, and ``sampler.guidance_chunk_rows`` against the three expressions
it replaces.  The run is a recording stand-in (``sampler._open_run`` is patched to return it), ``last_step_attention`` and
``weg.weg_update`` are recording stand-ins, the denoiser is a differentiable one-liner.

The expected sequences are literals written down from the three hand-written loops these drivers replaced.  Two places differ from those
loops on purpose and are marked DIFFERENCE 1 / DIFFERENCE 2 where they are asserted:
1. with the attention ring kept, the word-excitation loop no longer makes a side-engine forward at the last iteration (its result was
   overwritten by the ring's dict);
2. consecutive iterations with no host work between them are replayed as one ``steps(k)``, not as k times ``steps(1)``."""
import pytest
import torch

from convofusion_amd import _lib, sampler, scheduler, weg

YAML = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
G, S = 7, (3, 5, 4, 2, 1)

# shorthands of the recorded calls
I, R, RC, W, AD, CL = ("inpaint",), ("read", False), ("read", True), ("write",), ("attention_dict",), ("close",)
CH = [I, R, W]      # a changed iteration up to its write


def St(n):
    return ("steps", n)


def M(t):
    return ("maps", t)


class FakeRun:
    """Records what reaches the library, as ``SamplingRun`` would pass it on: ``steps(0)`` replays nothing and ``close()`` of a run that
    ``read(close=True)`` or an earlier ``close()`` has closed does nothing, so neither is recorded; a count the library would refuse
    fails here too."""
    device = torch.device("cpu")

    def __init__(self, table, first_iteration=0, ring=False, B=1, L=4):
        self.timesteps = [int(t) for t in table][first_iteration:]
        self.N, self.first_iteration, self.B, self.L = len(self.timesteps), first_iteration, B, L
        self.att_ring = ["ring"] if ring else None
        self.position, self.open, self.calls, self.written = 0, True, [], []
        self.latents = torch.randn((B, L, 128), generator=torch.Generator().manual_seed(3))

    def steps(self, n):
        assert self.open and 0 <= n and self.position + n <= self.N, (n, self.position, self.N)
        if n:
            self.calls.append(("steps", int(n)))
            self.position += n

    def read(self, close=False):
        assert self.open
        self.calls.append(("read", bool(close)))
        self.open = not close
        return self.latents.clone()

    def write(self, latents):
        assert self.open and not latents.requires_grad
        self.calls.append(("write",))
        self.written.append(latents.clone())
        self.latents = latents.clone()

    def inpaint(self):
        assert self.open
        self.calls.append(("inpaint",))

    def attention_dict(self):
        self.calls.append(("attention_dict",))
        return {"ring": self.position}

    def close(self):
        if self.open:
            self.calls.append(("close",))
            self.open = False


class FakeDenoiser:
    """Differentiable stand-in: (sample * 0.5, None); records how it was called."""

    def __init__(self):
        self.return_attention = "kept"
        self.calls = []

    def __call__(self, sample, timestep, encoder_hidden_states, mem_mask_dict, side_engine):
        self.calls.append(dict(timestep=timestep, rows=int(sample.shape[0]), memory_rows=[int(e.shape[0]) for e in encoder_hidden_states],
                               side_engine=side_engine, return_attention=self.return_attention, grad=torch.is_grad_enabled()))
        return sample * 0.5, None


def ddpm():
    return scheduler.DDPMScheduler(variance_type="fixed_small", clip_sample=True, **YAML)


def batch(B=1, with_masks=True):
    g = torch.Generator().manual_seed(5)
    enc = [torch.randn((G * B, s, 4), generator=g) for s in S]
    masks = {n: (torch.rand((G * B, s), generator=g) > 0.5) for n, s in zip(_lib.MEM_NAMES, S)} if with_masks else None
    return enc, masks


@pytest.fixture
def stage(monkeypatch):
    """Patches ``_open_run`` and ``last_step_attention``; ``stage.open(run)`` sets the run the next entry point gets."""
    class Stage:
        run, opened, maps_raises_at = None, [], None

        def open(self, run):
            self.run = run
            return run
    st = Stage()
    st.opened = []

    def open_run(denoiser, sch, enc, masks, B, L, num_inference_steps, want_ring, **kw):
        st.opened.append(dict(want_ring=want_ring, B=B, L=L, num_inference_steps=num_inference_steps, kw=kw))
        return st.run

    def maps(run, denoiser, t, enc, masks, guidance_chunks=sampler.CFG_CHUNKS, row_maps=None):
        assert run is st.run and guidance_chunks == G and row_maps is None
        run.calls.append(("maps", int(t)))
        if st.maps_raises_at == int(t):
            raise RuntimeError("maps")
        return f"att{int(t)}"
    monkeypatch.setattr(sampler, "_open_run", open_run)
    monkeypatch.setattr(sampler, "last_step_attention", maps)
    return st


# ---- sample

def sample_expected(T, mode, ring):
    """The parent's four arms, for a run over the executed timesteps T."""
    n = len(T)
    if not mode:
        return [St(n), RC], None
    if mode in ("all", "auto") and ring:
        return [St(n), R, AD, CL], {"ring": n}
    if mode == "all":
        return [c for t in T for c in (M(t), St(1))] + [RC], {t: f"att{t}" for t in T}
    att = f"att{T[-1]}"
    return [St(n - 1), M(T[-1]), St(1), RC], ({T[-1]: att} if mode == "auto" else att)


@pytest.mark.parametrize("ring", (False, True))
@pytest.mark.parametrize("mode", (False, True, "all", "auto"))
@pytest.mark.parametrize("n_steps,first", ((4, 0), (5, 2)))
def test_sample_call_sequence(stage, n_steps, first, mode, ring):
    sch = ddpm()
    touched = []
    sch.set_timesteps = lambda n: touched.append(n)
    run = stage.open(FakeRun(sch.timestep_table(n_steps)[1], first, ring))
    assert run.timesteps == ([750, 500, 250, 0] if n_steps == 4 else [400, 200, 0])
    enc, masks = batch()
    out = sampler.sample(FakeDenoiser(), sch, enc, masks, B=1, L=4, num_inference_steps=n_steps, return_attention=mode)
    want_calls, want_att = sample_expected(run.timesteps, mode, ring)
    assert run.calls == want_calls
    assert stage.opened[0]["want_ring"] == (mode in ("all", "auto"))
    assert touched == ([n_steps] if mode else [])           # no attention: the scheduler object is not touched
    if mode:
        assert torch.equal(out[0], run.latents) and out[1] == want_att
    else:
        assert torch.equal(out, run.latents)


# ---- sample_with_weg

WEG_A = dict(scale_factor=100, scale_range=[1.0, 0.5], max_iter_to_alter=2, thresholds={3: 0.16}, max_refinement_steps=3)
WEG_B = dict(WEG_A, thresholds={})
WEG_C = dict(WEG_A, max_iter_to_alter=5)
WEG_D = dict(WEG_A, max_iter_to_alter=1, thresholds={4: 0.16})
T5 = [800, 600, 400, 200, 0]
RING_END = [R, AD, CL]

# (parameters, return_attention, ring) -> the recorded calls
WEG_SEQUENCES = {
    # A: two changed, one skipped with the carry advanced, one threshold iteration, DONE before the last
    ("A", False, False): CH + [St(1)] + CH + [St(1), St(1)] + CH + [St(1), St(1), RC],
    ("A", True, False): CH + [St(1)] + CH + [St(1), St(1)] + CH + [St(1), M(0), St(1), RC],
    ("A", "auto", False): CH + [St(1)] + CH + [St(1), St(1)] + CH + [St(1), M(0), St(1), RC],
    ("A", "all", False): CH + [M(800), St(1)] + CH + [M(600), St(1), M(400), St(1)] + CH + [M(200), St(1), M(0), St(1), RC],
    ("A", "all", True): CH + [St(1)] + CH + [St(1), St(1)] + CH + [St(1), St(1)] + RING_END,
    ("A", "auto", True): CH + [St(1)] + CH + [St(1), St(1)] + CH + [St(1), St(1)] + RING_END,
    # B: DONE right after iteration 1
    ("B", False, False): CH + [St(1)] + CH + [St(1), St(3), RC],
    ("B", True, False): CH + [St(1)] + CH + [St(1), St(2), M(0), St(1), RC],
    ("B", "auto", False): CH + [St(1)] + CH + [St(1), St(2), M(0), St(1), RC],
    ("B", "all", False): CH + [M(800), St(1)] + CH + [M(600), St(1), M(400), St(1), M(200), St(1), M(0), St(1), RC],
    ("B", "all", True): CH + [St(1)] + CH + [St(1), St(3)] + RING_END,
    ("B", "auto", True): CH + [St(1)] + CH + [St(1), St(3)] + RING_END,
    # C: the loop reaches the last iteration
    ("C", False, False): (CH + [St(1)]) * 5 + [RC],
    ("C", True, False): (CH + [St(1)]) * 4 + CH + [M(0), St(1), RC],
    ("C", "auto", False): (CH + [St(1)]) * 4 + CH + [M(0), St(1), RC],
    ("C", "all", False): [c for t in T5 for c in CH + [M(t), St(1)]] + [RC],
    # DIFFERENCE 1: the parent made M(0) before the last replay here and dropped its result for the ring's dict
    ("C", "all", True): (CH + [St(1)]) * 5 + RING_END,
    ("C", "auto", True): (CH + [St(1)]) * 5 + RING_END,
    # D: DIFFERENCE 2: the three skipped iterations 1 - 3 go out as St(3); the parent made St(1) three times
    ("D", False, False): CH + [St(1), St(3)] + CH + [St(1), RC],
}
# what each weg_update call was given: (i, t, num_steps, scale_carry at the call, same_memories), with carry_scale_range=True
WEG_CALLS = {
    "A": [(0, 800, 5, [1.0, 0.5], False), (1, 600, 5, [1.0, 0.875], True), (3, 200, 5, [1.0, 0.9921875], True)],
    "B": [(0, 800, 5, [1.0, 0.5], False), (1, 600, 5, [1.0, 0.875], True)],
    "C": [(0, 800, 5, [1.0, 0.5], False), (1, 600, 5, [1.0, 0.875], True), (2, 400, 5, [1.0, 0.96875], True),
          (3, 200, 5, [1.0, 0.9921875], True), (4, 0, 5, [1.0, 0.998046875], True)],
    "D": [(0, 800, 5, [1.0, 0.5], False), (4, 0, 5, [1.0, 0.998046875], True)],
}


@pytest.fixture
def weg_calls(monkeypatch):
    """``weg.weg_update`` replaced: records its arguments, advances the carried scale table as the real one does, returns latents * 2 (exact)."""
    calls = []

    def weg_update(denoiser, latents, i, t, states, masks, focus_indices, params, num_steps, scale_carry=None, same_memories=False):
        calls.append((i, int(t), num_steps, None if scale_carry is None else [float(v) for v in scale_carry], same_memories))
        assert [int(s.shape[0]) for s in states] == [1] * 5 and all(m.dtype == torch.uint8 for m in masks.values())
        weg.scale_range_schedule(params, num_steps, i, scale_carry)
        if getattr(weg_update, "raises_at", None) == i:
            raise RuntimeError("weg_update")
        return latents * 2.0, 0.0
    monkeypatch.setattr(weg, "weg_update", weg_update)
    calls_and_fn = (calls, weg_update)
    return calls_and_fn


@pytest.mark.parametrize("carry", (True, False))
@pytest.mark.parametrize("case,mode,ring", sorted(WEG_SEQUENCES, key=str))
def test_sample_with_weg_call_sequence(stage, weg_calls, case, mode, ring, carry):
    sch = ddpm()
    run = stage.open(FakeRun(sch.timestep_table(5)[1], 0, ring))
    assert run.timesteps == T5
    base = run.latents.clone()
    enc, masks = batch()
    params = dict(A=WEG_A, B=WEG_B, C=WEG_C, D=WEG_D)[case]
    out = sampler.sample_with_weg(FakeDenoiser(), sch, enc, masks, [[1, 2]], params, B=1, L=4, num_inference_steps=5,
                                  return_attention=mode, carry_scale_range=carry)
    assert run.calls == WEG_SEQUENCES[case, mode, ring]
    want = WEG_CALLS[case]
    assert weg_calls[0] == (want if carry else [(i, t, n, None, same) for i, t, n, _, same in want])
    assert [torch.equal(w, base * 2.0 ** (k + 1)) for k, w in enumerate(run.written)] == [True] * len(want)
    assert stage.opened[0]["want_ring"] == (mode in ("all", "auto"))
    assert [int(t) for t in sch.timesteps] == T5         # sample_with_weg sets the scheduler's table, whatever the mode
    lat = out[0] if mode else out
    assert torch.equal(lat, base * 2.0 ** len(want))
    if mode:
        assert out[1] == ({"ring": 5} if ring else {t: f"att{t}" for t in T5} if mode == "all" else "att0" if mode is True else {0: "att0"})


# ---- sample_with_loss_guidance

def quadratic(x0):
    return 0.5 * (x0 * x0).sum()


def x0_factor(sch, t):
    """x0_hat = k x for the stand-in denoiser: every chunk predicts 0.5 x, so the guidance combine is 0.5 x."""
    a = float(sch.alphas_cumprod[int(t)])
    return (1.0 - 0.5 * (1.0 - a) ** 0.5) / a ** 0.5


LOSS_SEQUENCES = {
    None: (CH + [St(1)]) * 4 + [RC],
    # DIFFERENCE 2: un-guided iterations in a row go out as one steps(k); the parent made steps(1) four times
    (): [St(4), RC],
    (1, 3): [St(1)] + CH + [St(1), St(1)] + CH + [St(1), RC],
}


@pytest.mark.parametrize("step_size", ("number", "list", "callable"))
@pytest.mark.parametrize("guided", (None, (), (1, 3)))
def test_sample_with_loss_guidance_call_sequence_and_update(stage, guided, step_size):
    sch, den = ddpm(), FakeDenoiser()
    B = 2
    run = stage.open(FakeRun(sch.timestep_table(4)[1], 0, False, B=B))
    T = run.timesteps
    base = run.latents.clone()
    enc, masks = batch(B)
    asked = []
    steps = {"number": 0.125, "list": [0.5, 0.25, 0.125, 0.0625], "callable": lambda i, t: asked.append((i, t)) or 0.03125 * (i + 1)}[step_size]
    size = {"number": lambda i: 0.125, "list": lambda i: steps[i], "callable": lambda i: 0.03125 * (i + 1)}[step_size]
    out = sampler.sample_with_loss_guidance(den, sch, enc, masks, quadratic, steps, B=B, L=4, num_inference_steps=4, guided_iterations=guided)
    assert run.calls == LOSS_SEQUENCES[guided]
    its = list(range(4)) if guided is None else list(guided)
    # the written latents: x - step * grad, grad of 0.5 |k x|^2 = k^2 x (float32 arithmetic of a handful of operations: 1e-5)
    x = base
    for n, i in enumerate(its):
        x = x - size(i) * x0_factor(sch, T[i]) ** 2 * x
        assert torch.allclose(run.written[n], x, rtol=1e-5, atol=1e-6)
        x = run.written[n]
    assert len(run.written) == len(its) and torch.equal(out, x)
    if step_size == "callable":
        assert asked == [(i, T[i]) for i in its]
    # the forwards: the six chunks of non-zero weight, on the side engine, under enable_grad, attention off -- and restored afterwards
    assert den.calls == [dict(timestep=T[i], rows=6 * B, memory_rows=[6 * B] * 5, side_engine=True, return_attention=False, grad=True) for i in its]
    assert den.return_attention == "kept"
    assert stage.opened[0]["want_ring"] is False


# ---- exceptions

def test_exception_in_weg_update_closes_the_run(stage, weg_calls):
    sch = ddpm()
    run = stage.open(FakeRun(sch.timestep_table(5)[1]))
    weg_calls[1].raises_at = 1
    with pytest.raises(RuntimeError, match="weg_update"):
        sampler.sample_with_weg(FakeDenoiser(), sch, *batch(), [[1, 2]], WEG_C, B=1, L=4, num_inference_steps=5)
    assert run.calls == CH + [St(1), I, R, CL] and not run.open


def test_exception_in_loss_closes_the_run_and_restores_return_attention(stage):
    sch, den = ddpm(), FakeDenoiser()
    run = stage.open(FakeRun(sch.timestep_table(4)[1], B=2))

    def loss(x0):
        raise RuntimeError("loss")
    with pytest.raises(RuntimeError, match="loss"):
        sampler.sample_with_loss_guidance(den, sch, *batch(2), loss, 0.1, B=2, L=4, num_inference_steps=4, guided_iterations=(2,))
    assert run.calls == [St(2), I, R, CL] and not run.open      # (DIFFERENCE 2: St(2) was St(1) twice)
    assert den.return_attention == "kept"


@pytest.mark.parametrize("loop", ("sample", "weg"))
def test_exception_in_maps_closes_the_run(stage, weg_calls, loop):
    sch = ddpm()
    run = stage.open(FakeRun(sch.timestep_table(5)[1]))
    stage.maps_raises_at = 600
    with pytest.raises(RuntimeError, match="maps"):
        if loop == "sample":
            sampler.sample(FakeDenoiser(), sch, *batch(), B=1, L=4, num_inference_steps=5, return_attention="all")
        else:
            sampler.sample_with_weg(FakeDenoiser(), sch, *batch(), [[1, 2]], WEG_C, B=1, L=4, num_inference_steps=5, return_attention="all")
    assert run.calls == ([M(800), St(1), M(600), CL] if loop == "sample" else CH + [M(800), St(1)] + CH + [M(600), CL]) and not run.open


# ---- guidance_chunk_rows against the three expressions it replaces

def parent_last_chunk(enc, cond_masks, G, B, row_maps):
    if row_maps is not None:
        idx = [m[(G - 1) * B:].long() for m in row_maps]
        states = [e.index_select(0, i.to(e.device)) for e, i in zip(enc, idx)]
        masks = {k: (v.index_select(0, idx[_lib.MEM_NAMES.index(k)].to(v.device)) if v is not None else None) for k, v in (cond_masks or {}).items()}
    else:
        states = [e.chunk(G)[-1] for e in enc]
        masks = {k: (v.chunk(G)[-1] if v is not None else None) for k, v in (cond_masks or {}).items()}
    return states, masks


def parent_text_chunk(enc, cond_masks, G, B, rm):
    if rm is not None:
        idx = [m[B:2 * B].long() for m in rm]
        text_states = [e.index_select(0, i.to(e.device)).contiguous() for e, i in zip(enc, idx)]
        text_masks = {k: (v.index_select(0, idx[_lib.MEM_NAMES.index(k)].to(v.device)).to(torch.uint8).contiguous() if v is not None else v)
                      for k, v in (cond_masks or {}).items()}
    else:
        text_states = [e.chunk(G)[1] for e in enc]
        text_masks = {k: (v.chunk(G)[1].to(torch.uint8).contiguous() if v is not None else v) for k, v in (cond_masks or {}).items()}
    return text_states, text_masks


def parent_weighted_chunks(enc, cond_masks, G, B, rm, chunks):
    if rm is not None:
        idx = [torch.cat([m[c * B:(c + 1) * B] for c in chunks]).long() for m in rm]
        states = [e.index_select(0, i.to(e.device)).detach().contiguous() for e, i in zip(enc, idx)]
        masks = {k: (v.index_select(0, idx[_lib.MEM_NAMES.index(k)].to(v.device)).contiguous() if v is not None else v)
                 for k, v in (cond_masks or {}).items()}
    else:
        states = [torch.cat([e.chunk(G)[c] for c in chunks]).detach().contiguous() for e in enc]
        masks = {k: (torch.cat([v.chunk(G)[c] for c in chunks]).contiguous() if v is not None else v) for k, v in (cond_masks or {}).items()}
    return states, masks


def same(got, want):
    (gs, gm), (ws, wm) = got, want
    assert len(gs) == len(ws) == 5 and list(gm) == list(wm)
    for g, w in zip(gs, ws):
        assert g.dtype == w.dtype and g.device == w.device and torch.equal(g, w)
    for k in wm:
        assert (gm[k] is None) == (wm[k] is None)
        if wm[k] is not None:
            assert gm[k].dtype == wm[k].dtype and torch.equal(gm[k], wm[k])


def guidance_batches():
    """(memories, masks, row maps) at G = 7, B = 2: the replicated batch and a ``build_guidance_batch`` batch with maps, each with one
    None mask, and each once more with cond_masks=None."""
    B = 2
    enc, masks = batch(B)
    masks["alsn"] = None
    g = torch.Generator().manual_seed(9)
    cond, uncond = [torch.randn((B, s, 4), generator=g) for s in S], [torch.randn((1, s, 4), generator=g) for s in S]
    cm = {n: (torch.rand((B, s), generator=g) > 0.5) for n, s in zip(_lib.MEM_NAMES, S)}
    cm["apb"] = None
    u_enc, maps, u_masks = sampler.build_guidance_batch(cond, uncond, cm, None)
    assert u_masks["apb"] is None and [int(m.numel()) for m in maps] == [G * B] * 5
    return [(enc, masks, None), (enc, None, None), (u_enc, u_masks, maps), (u_enc, None, maps)]


@pytest.mark.parametrize("which", range(4))
def test_guidance_chunk_rows_equals_the_three_expressions(which):
    B = 2
    enc, masks, maps = guidance_batches()[which]
    rows = sampler.guidance_chunk_rows
    same(rows(enc, masks, [G - 1], G, B, maps), parent_last_chunk(enc, masks, G, B, maps))
    st, mk = rows(enc, masks, [1], G, B, maps)
    same((st, {k: (v.to(torch.uint8).contiguous() if v is not None else v) for k, v in mk.items()}), parent_text_chunk(enc, masks, G, B, maps))
    for chunks in ([0, 1, 2, 3, 4, 5], [0, 6], [0, 2, 5], [0]):
        st, mk = rows(enc, masks, chunks, G, B, maps)
        same(([s.detach() for s in st], mk), parent_weighted_chunks(enc, masks, G, B, maps, chunks))
    if masks is None:
        assert rows(enc, None, [1], G, B, maps)[1] == {}
