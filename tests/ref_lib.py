"""Loader for the compiled reference modules of oracle/_ref (built by oracle/build_ref.py from __graft_entry__.build()).

TEST INFRASTRUCTURE.  It reads only oracle/_ref -- never the reference tree, which the GPU machine does not have; the binaries
travel there with the working tree.  So that a broken build cannot hide behind a skip:
    manifest says built: false          -> pytest.skip with the manifest's reason (a checkout without the reference tree)
    manifest missing                    -> failure (build() always writes one)
    built: true, module absent/broken   -> failure
"""
import importlib.util
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
_modules = {}


def manifest(ref_dir=REF_DIR):
    path = os.path.join(ref_dir, "manifest.json")
    if not os.path.isfile(path):
        pytest.fail(f"{path} is missing: __graft_entry__.build() writes it whether or not the reference can be built")
    with open(path) as f:
        return json.load(f)


def load(name, ref_dir=REF_DIR):
    """The extension module `name` (_ref_raymarching, _ref_raymarching_fmad, _ref_chamfer) of `ref_dir`."""
    key = (os.path.abspath(ref_dir), name)
    if key in _modules:
        return _modules[key]
    m = manifest(ref_dir)
    if not m.get("built"):
        pytest.skip(f"compiled reference not built: {m.get('reason', 'no reason recorded')}")
    import torch  # noqa: F401  (the extension links against libtorch: it has to be loaded first)
    path = os.path.join(ref_dir, m.get("modules", {}).get(name, name + ".so"))
    if not os.path.isfile(path):
        pytest.fail(f"oracle/_ref/manifest.json says built, but {path} is missing")
    try:
        spec = importlib.util.spec_from_file_location(name, path)  # the name must equal the build name (PyInit_<name>)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    except Exception as e:  # noqa: BLE001
        pytest.fail(f"oracle/_ref/manifest.json says built, but {path} does not import: {e!r}")
    sys.modules.setdefault(name, mod)
    _modules[key] = mod
    return mod
