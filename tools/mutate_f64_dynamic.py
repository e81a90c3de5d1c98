"""Do the float64 pins of the space-time encoders notice a wrong reference?  (needs a HIP device)

    python tools/mutate_f64_dynamic.py            # all five variants
    python tools/mutate_f64_dynamic.py swap_blend # one of them

Each variant applies ONE error to a temporary copy of tests/torch_f64_dynamic.py -- never to a kernel, never to the committed file --
and runs the tests of tests/test_dynamic_f64_gpu.py that it concerns against the unchanged kernels with that copy imported in the
restatement's place.  A variant is "caught" when at least one test fails; the script prints which tests did and exits non-zero if a
variant passes everything.  Every edit must match the restatement's text exactly once (or the stated number of times), so a variant
that silently stops applying fails here instead of counting as caught.
"""
import importlib.util
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
SOURCE = os.path.join(TESTS, "torch_f64_dynamic.py")

_CONSTANTS = "    k1, k2, b_lo, b_hi, lag = time_constants(t_host, time_resolution, reciprocal_division)\n"
# name: (pytest -k selection, [(text, replacement, occurrences)])
VARIANTS = {
    "swap_blend": ("hash", [(_CONSTANTS, _CONSTANTS.replace("b_lo, b_hi", "b_hi, b_lo"), 2)]),
    "drop_lagrange": ("hash or flow_grid", [
        (_CONSTANTS, _CONSTANTS + "    lag = lag[:3] + [0.0]\n", 2),
        ("    w = lagrange_weights_host(t_host, 4, reciprocal_division)\n", "    w = lagrange_weights_host(t_host, 4, reciprocal_division)[:3] + [0.0]\n", 1)]),
    "grad_at_clamp": ("planes", [("float(R - 1) * inside.to(dtype) * (carrier - carrier.detach())", "float(R - 1) * (carrier - carrier.detach())", 1)]),
    "floor_f64": ("planes", [("    f0 = torch.floor(u)\n", "    f0 = torch.floor(torch.clamp(p32.double() * float(R - 1), 0.0, float(R - 1))).float()\n", 1)]),
    "blend_quarter": ("planes_multi", [("0.5 * outs[1] + 0.25 * (outs[2] + outs[3])", "0.25 * outs[1] + 0.25 * (outs[2] + outs[3])", 1)]),
}


def mutated_source(name):
    text = open(SOURCE).read()
    for old, new, count in VARIANTS[name][1]:
        if text.count(old) != count:
            raise SystemExit(f"{name}: the restatement no longer holds {old!r} {count} time(s): update this variant")
        text = text.replace(old, new)
    return text


def run_variant(name):
    """In a child process: import the mutated copy as `torch_f64_dynamic`, then run the selected tests; returns the failed test ids."""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "torch_f64_dynamic.py")
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
    spec = importlib.util.spec_from_file_location("torch_f64_dynamic", path)
    module = importlib.util.module_from_spec(spec)
    sys.modules["torch_f64_dynamic"] = module
    spec.loader.exec_module(module)
    return pytest.main([os.path.join(TESTS, "test_dynamic_f64_gpu.py"), "-m", "gpu", "-q", "--tb=no", "-rf", "-k", selection])


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
