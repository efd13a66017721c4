"""Static checks of bench.py that run without a GPU.  The driver's command is the one run nobody re-checks by hand: a name
released with `del` and read again further down (round 3: the pipeline object, read while assembling the JSON line) only shows
up at the very end of a several-minute GPU run."""
import ast
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _functions(tree):
    return [n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))]


def test_no_name_is_read_after_it_was_deleted():
    src = open(os.path.join(ROOT, "bench.py")).read()
    tree = ast.parse(src)
    problems = []
    for fn in _functions(tree):
        deleted = {}      # name -> line of the `del`
        events = []
        for node in ast.walk(fn):
            if isinstance(node, ast.Name):
                events.append((node.lineno, node.col_offset, type(node.ctx).__name__, node.id))
        for line, col, ctx, name in sorted(events):
            if ctx == "Del":
                deleted[name] = line
            elif ctx == "Store":
                deleted.pop(name, None)
            elif ctx == "Load" and name in deleted and line > deleted[name]:
                problems.append(f"{fn.name}: `{name}` deleted at line {deleted[name]}, read at line {line}")
    assert not problems, "\n".join(problems)


def test_the_json_line_carries_the_contract_fields():
    src = open(os.path.join(ROOT, "bench.py")).read()
    for key in ("metric=", "value=", "unit=", "n_gpus=", "steps=", "warmup=", "ms_per_step=", "higher_is_better=", "scaling=",
                "vs_baseline=", "dtype=", "data=", "config=", "roofline=", "cpu_baseline="):
        assert key in src, key
    # roofline / cpu_baseline objects: the fields the contract names
    for key in ("bound=", "achieved=", "peak=", "frac=", "traffic=", "cores=", "kind=", "sample="):
        assert key in src, key


def _run_bench(args, env=None, timeout=300):
    import subprocess
    import sys
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, env=e)


def test_gpus_flag_and_launcher_world_must_agree():
    """`bench.py --gpus N` started without a launcher used to run one rank and report n_gpus: 1.  Now a launcher
    world that differs from --gpus is an error, and --gpus N > 1 without a launcher re-executes under torch.distributed.run --
    or fails loudly when the node has fewer GPUs (here: none)."""
    r = _run_bench(["--gpus", "1"], env={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "must agree" in r.stderr, r.stderr[-500:]
    r = _run_bench(["--gpus", "4"])
    assert r.returncode != 0 and "GPU(s) are visible" in r.stderr, r.stderr[-500:]


def test_the_json_line_is_the_only_thing_on_stdout_when_a_collective_library_is_loaded():
    """RCCL prints a version banner on C stdout (flushed at exit, after the line): bench.py keeps a private handle on the real
    stdout for its ONE line and points descriptor 1 at stderr before any process group exists."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert src.count("print(") == 1 and "print(json.dumps(out), file=line_out)" in src
    i_dup, i_init = src.index("os.dup2(2, 1)"), src.index("dist.init_process_group(")
    assert i_dup < i_init
    assert "line_out = os.fdopen(os.dup(1), \"w\")" in src and "line_out.flush()" in src


def test_launch_shape_rules_of_the_timed_pass():
    """Round 6: the model order and the pairs per launch are chosen by rules measured on the pipelined job
    (profiles/r6_experiments.txt C20): ordered model from 32 768 Gaussians, four pairs per launch with it, two without;
    explicit arguments win; the sub-lines resolve the rule for THEIR model."""
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from gs2mesh_amd.rasterizer import auto_blend_mode, auto_cull_level, auto_spatial_order
    assert not auto_spatial_order(10_000) and auto_spatial_order(32_768) and auto_spatial_order(300_000) and auto_spatial_order(2_000_000)
    assert auto_cull_level(300_000) == 1 and auto_cull_level(2_000_000) == 2
    auto = types.SimpleNamespace(spatial_order=-1, pairs_per_launch=0)
    assert bench.spatial_order_for(auto, 300_000) and not bench.spatial_order_for(auto, 10_000)
    assert bench.pairs_per_launch_for(auto, 300_000) == 4 and bench.pairs_per_launch_for(auto, 10_000) == 2
    unordered = types.SimpleNamespace(spatial_order=0, pairs_per_launch=0)
    assert bench.pairs_per_launch_for(unordered, 2_000_000) == 2
    fixed = types.SimpleNamespace(spatial_order=-1, pairs_per_launch=1, ppl_arg=2)          # main() resolved 2 -> sub-lines see the argument as given
    assert bench.pairs_per_launch_for(fixed, 300_000) == 2
    import numpy as np
    assert auto_blend_mode(dict(opacity=np.array([5.0, 5.0, -1.0, 0.0], np.float32), raw=True)) == 3      # half of them above logit(0.98)
    assert auto_blend_mode(dict(opacity=np.array([0.5, 0.97], np.float32))) == 2


def test_plain_and_full_options_are_declared():
    """`--full` switches the diagnostics on, `--dump-outputs DIR` writes the last step's outputs; both parse without a GPU."""
    r = _run_bench(["--help"], timeout=120)
    assert r.returncode == 0, r.stderr[-500:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout and "--steps" in r.stdout
