"""CPU: the frozen parts of bench.py's contract -- checked on the source, no GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src():
    return open(os.path.join(ROOT, "bench.py")).read()


def test_bench_step_is_frozen_at_1024_interleaved_steps():
    s = _src()
    m = re.search(r'add_argument\("--transitions", type=int, default=(\d+)', s)
    assert m and int(m.group(1)) == 1024
    m = re.search(r'add_argument\("--thin", type=int, default=(\d+)', s)
    assert m and int(m.group(1)) == 2                      # the reference's sample_chain thinning
    m = re.search(r'add_argument\("--chains", type=int, default=(\d+)', s)
    assert m and int(m.group(1)) == 65536                  # BASELINE.json's headline chain count
    m = re.search(r'add_argument\("--gpus", type=int, default=(\d+)', s)
    assert m and int(m.group(1)) == 1


def test_bench_reports_the_transport_it_used():
    s = _src()
    assert '"dist_backend"' in s and '"ranks"' in s
    # rccl_ranks is only emitted under the nccl backend
    assert re.search(r'if backend == "nccl":\n\s+line\["rccl_ranks"\]', s)


def test_oracle_only_in_the_cpu_baseline_leg():
    s = _src()
    for m in re.finditer(r"^\s*import oracle|^\s*from oracle", s, flags=re.M):
        # inside cpu_baseline() or the child-process code string it builds
        head = s[:m.start()]
        assert head.rfind("def cpu_baseline(") > head.rfind("\ndef main("), "oracle imported outside the cpu_baseline leg"


def test_bench_launches_its_own_ranks_when_asked_for_more_than_one_gpu():
    """`python bench.py --gpus 2` outside a launcher starts torch.distributed.run as a CHILD process (before anything
    touched the GPU) and leaves with its return code: on this GPU-less box the two ranks fail with torch's own "no GPU"
    error, and the parent no longer refuses with `--gpus 2 but WORLD_SIZE=1`."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       env=env, cwd=ROOT, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        assert r.returncode == 0
        return
    assert r.returncode != 0
    assert "but WORLD_SIZE=" not in r.stderr
    if not torch.cuda.is_available():
        assert "No HIP GPUs are available" in r.stderr or "Found no NVIDIA driver" in r.stderr or "no GPU" in r.stderr.lower(), r.stderr[-1500:]
        assert "torch.distributed.elastic" in r.stderr or "ChildFailedError" in r.stderr      # the failure came from the children


def test_stdout_line_is_short_and_the_rest_goes_to_the_extras_file():
    """Round 5's line grew past what the driver's parser reads (BENCH_r05.json: parsed null).  The line is built from a
    fixed short key set and bench.py refuses to print one of 4 KB or more; the long figures go to --extras; nothing the CLI
    flows print reaches either stream by default.  (tests/test_gpu_scaling.py::test_bench_stdout_is_one_json_line runs it.)"""
    s = _src()
    assert "assert len(text) < 4096" in s
    assert 'add_argument("--extras"' in s and 'add_argument("--verbose"' in s
    assert 'sys.stdout = sys.stderr if args.verbose else open(os.devnull, "w")' in s
    line_block = s[s.index("        line = {"):s.index("        # ---- everything else: bench_extras.json")]
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "workload", "roofline", "ess_per_sec", "ranks", "dist_backend",
              "cpu_baseline", "bound", "achieved", "peak", "frac", "traffic", "kernel_ms"):
        assert '"%s"' % k in line_block, k
    for k in ("other_models", "vi_kernel", "german_credit", "election", "strong_shard", '"profile"', '"note"'):
        assert k not in line_block, k
    # exactly one print to the real stdout
    assert len(re.findall(r"file=json_out", s)) == 1


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_dump_outputs_fits_the_budget_and_samples_reproducibly(tmp_path, monkeypatch):
    """--dump-outputs: small arrays whole (float32 / counts as float64), an array over its share of the budget as a
    seeded sample of its flattened elements, everything together within the budget, the same files on a second call."""
    import numpy as np
    import torch
    b = _bench_module()
    monkeypatch.setattr(b, "DUMP_BUDGET_BYTES", 100000)
    g = torch.Generator().manual_seed(0)
    arrays = {"q": torch.randn(64, 71, generator=g), "logp": torch.randn(64, generator=g),
              "accept_count": torch.randint(0, 1000, (64,), dtype=torch.int32, generator=g),
              "trace": torch.randn(16, 64, 71, generator=g)}
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), arrays, seed=3)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["accept_count.npy", "logp.npy", "q.npy", "trace_sample.npy"]
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)), n
    q, acc = np.load(tmp_path / "a" / "q.npy"), np.load(tmp_path / "a" / "accept_count.npy")
    assert q.dtype == np.float32 and np.array_equal(q, arrays["q"].numpy())
    assert acc.dtype == np.float64 and np.array_equal(acc, arrays["accept_count"].numpy())
    flat = arrays["trace"].numpy().reshape(-1)
    total = sum(np.load(tmp_path / "a" / n).nbytes for n in names)
    assert total <= 100000
    share = (100000 - (q.nbytes + acc.nbytes + 64 * 4)) // 4
    idx = np.unique(np.random.RandomState(3).randint(0, flat.size, size=share, dtype=np.int64))
    assert np.array_equal(np.load(tmp_path / "a" / "trace_sample.npy"), flat[idx])


def test_plain_run_leaves_the_secondary_figures_to_full():
    s = _src()
    assert 'add_argument("--full", action="store_true"' in s and 'add_argument("--dump-outputs"' in s
    assert "secondary = args.full and" in s and "if world > 1 and args.full:" in s
    assert "if args.full and world == 1 and not args.no_cpu_baseline:" in s


def test_issue_mix_comes_from_the_newest_ledger():
    b = _bench_module()
    mix, src = b.headline_mix()
    assert src.startswith("profiles/r") and src.endswith("_headline_ledger.txt")
    assert set(mix) == set(b.HEADLINE_COST) and 1400 < sum(mix.values()) < 1700
