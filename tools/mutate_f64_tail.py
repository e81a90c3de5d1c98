"""Do the pins of the density tail and the flow MLP notice a wrong reference?  (needs a HIP device)

    python tools/mutate_f64_tail.py              # all six variants
    python tools/mutate_f64_tail.py swap_levels  # one of them

Each variant applies ONE error to a temporary copy of tests/torch_f64_tail.py -- never to a kernel, never to the committed file -- and
runs the tests of tests/test_dynamic_tail_gpu.py that it concerns against the unchanged kernels with that copy imported in the
restatement's place.  A variant is "caught" when at least one test fails; the script prints which tests did and exits non-zero if a
variant passes everything.  Every edit must match the restatement's text exactly once, so a variant that silently stops applying fails
here instead of counting as caught (tests/test_dynamic_tail_cpu.py checks the same without a device).
"""
import importlib.util
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
SOURCE = os.path.join(TESTS, "torch_f64_tail.py")

# name: (pytest -k selection, [(text, replacement)])
VARIANTS = {
    "swap_factors": ("forward or tail_fn", [("W_BASE, W_NEIGHBOUR = 0.5, 0.25", "W_BASE, W_NEIGHBOUR = 0.25, 0.5")]),
    "drop_half_rounding": ("forward_blend", [("bool(half[0] and half[1])", "False")]),
    "pad_zeros": ("forward or tail_fn", [("pad = torch.ones(row.shape[0]", "pad = torch.zeros(row.shape[0]")]),
    "no_clamp": ("tail_fn_random", [("_TruncExp.apply(h[:, 0])", "torch.exp(h[:, 0])")]),
    "swap_levels": ("tail_fn", [("order = list(range(hash_s.shape[0]))", "order = [l ^ 1 for l in range(hash_s.shape[0])]")]),
    "blended_half": ("tail_fn", [("_ScaleGrad.apply(plane_d.to(dtype), 1.0)", "_ScaleGrad.apply(plane_d.to(dtype), 0.5)")]),
}


def mutated_source(name):
    text = open(SOURCE).read()
    for old, new in VARIANTS[name][1]:
        if text.count(old) != 1:
            raise SystemExit(f"{name}: the restatement no longer holds {old!r} exactly once: update this variant")
        text = text.replace(old, new)
    return text


def run_variant(name):
    """In a child process: import the mutated copy as `torch_f64_tail`, then run the selected tests; returns the failed test ids."""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "torch_f64_tail.py")
        with open(path, "w") as f:
            f.write(mutated_source(name))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, VARIANTS[name][0]], cwd=ROOT, capture_output=True, text=True)
    failed = sorted({line.split(" ")[1] for line in out.stdout.splitlines() if line.startswith("FAILED ")})
    if out.returncode not in (0, 1):  # neither "all passed" nor "some failed": a crash, not a verdict
        sys.stdout.write(out.stdout[-4000:] + out.stderr[-4000:])
        raise SystemExit(f"{name}: the test run ended with status {out.returncode}")
    return failed


def child(path, selection):
    import pytest
    sys.path[:0] = [TESTS, os.path.join(ROOT, "selfsupervised-nvsf_amd"), ROOT]
    spec = importlib.util.spec_from_file_location("torch_f64_tail", path)
    module = importlib.util.module_from_spec(spec)
    sys.modules["torch_f64_tail"] = module
    spec.loader.exec_module(module)
    return pytest.main([os.path.join(TESTS, "test_dynamic_tail_gpu.py"), "-m", "gpu", "-q", "--tb=no", "-rf", "-k", selection])


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        sys.exit(child(sys.argv[2], sys.argv[3]))
    missed = []
    for variant in sys.argv[1:] or list(VARIANTS):
        failed = run_variant(variant)
        tests = sorted({f.split("::")[1].split("[")[0] for f in failed})
        print(f"{variant}: {len(failed)} cases failed in {', '.join(tests) if tests else 'NO TEST'}")
        if not failed:
            missed.append(variant)
    sys.exit(1 if missed else 0)
