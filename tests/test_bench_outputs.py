"""bench.py's own arguments: --steps / --warmup are checked before anything starts (CPU), --dump-outputs writes what the timed
path computed, and a plain run's line holds the headline figure while --full adds the rest (-m gpu)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("steps,warmup", [(0, 3), (20, -1), (990, 10)])
def test_bench_refuses_step_counts_it_cannot_time(steps, warmup):
    """One 1000-step run holds the warm-up, the timed iterations and the profiled forward: a count outside that is an argument
    error, not a shorter measurement."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 2 and "steps + warmup <= 999" in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_bench_dumps_the_latents_of_its_last_timed_step(tmp_path):
    """`bench.py --steps 2 --warmup 1 --dump-outputs DIR`: DIR/latents.npy holds the batch's latents after iteration 3 of the run --
    bit for bit what the same run on the same seeded weights and conditioning returns after 3 iterations."""
    import torch
    import bench
    from convofusion_amd import scheduler
    from convofusion_amd.sampler import SamplingRun
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--headline-only",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2 and line["warmup"] == 1
    assert sorted(os.listdir(out)) == ["latents.npy"]
    got = np.load(out / "latents.npy")
    assert got.dtype == np.float32 and got.shape == (bench.B_PER_GPU, bench.L, 128) and np.isfinite(got).all()

    dev = torch.device("cuda", 0)
    with torch.random.fork_rng(devices=[0]):
        m = bench.make_model(dev)
    mems, masks = bench.make_inputs(bench.B_PER_GPU, dev, seed=1234)
    sch = scheduler.DDPMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                  variance_type="fixed_small", clip_sample=True)
    with SamplingRun(m, sch, mems, masks, bench.B_PER_GPU, bench.L, 1000, guidance_scale=7.5, seed=0, first_utterance=0) as run:
        run.steps(3)
        want = run.read().cpu().numpy()
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_plain_bench_line_holds_the_headline_and_full_adds_the_rest():
    """A plain `bench.py --steps K --warmup W` measures the headline figure and nothing else; the profiled forward behind
    `kernel_classes` and the rooflines, the GPU state and the other measurements come with --full (--headline-only trims the latter)."""
    def line(*extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", *extra],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    profiled = {"roofline", "roofline_xattn", "roofline_step", "kernel_classes", "tflop_once_per_run_not_per_step", "gpu_state"}
    other = {"value_without_zero_weight_chunk", "value_split_pairs_everywhere", "full_loop_s", "other_configs", "c1_single_utterance", "cpu_baseline"}
    plain = line()
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= plain.keys()
    assert plain["higher_is_better"] is True and plain["steps"] == 2 and plain["warmup"] == 1
    assert abs(plain["value"] * plain["ms_per_step"] - 1000.0) < 1e-6
    assert not (profiled | other) & plain.keys()
    full = line("--full", "--headline-only")
    assert profiled <= full.keys() and full["kernel_classes"]["xattn"]["launches"] > 0
    assert full["value_without_zero_weight_chunk"] is None and full["full_loop_s"] is None
    assert not {"other_configs", "c1_single_utterance", "cpu_baseline"} & full.keys()
