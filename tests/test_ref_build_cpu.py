"""oracle/_ref after __graft_entry__.build(): the recipe (oracle/build_ref.py) and the loader's rule for absence (tests/ref_lib.py).
No GPU: the extension modules import on the CPU; nothing of them is run here."""
import json
import os
import sys

import pytest

import ref_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import build_ref  # noqa: E402

NAMES = ("_ref_raymarching", "_ref_raymarching_fmad", "_ref_chamfer")


def test_built_modules_import_and_export_the_reference_operators():
    """Where the reference tree was present at build(): built, three modules, exactly the ten + two functions of the reference's
    bindings, and nothing else left in oracle/_ref (no copied or translated source, no object file)."""
    mods = {name: ref_lib.load(name) for name in NAMES}  # skips where the manifest says why nothing was built
    m = ref_lib.manifest()
    assert m["built"] is True and set(m["modules"]) == set(NAMES)
    assert m["flags"] == {"_ref_raymarching": ["-ffp-contract=off"], "_ref_raymarching_fmad": [], "_ref_chamfer": ["-ffp-contract=off"]}
    assert len(m["sources"]) == 5 and all(len(d) == 64 for d in m["sources"].values()) and m["torch"] and m["hip"]
    for name, mod in mods.items():
        public = sorted(n for n in dir(mod) if not n.startswith("_"))
        assert public == sorted(build_ref.EXPORTS[name]), name
        assert all(callable(getattr(mod, n)) for n in public)
    assert len(build_ref.EXPORTS["_ref_raymarching"]) == 10 and len(build_ref.EXPORTS["_ref_chamfer"]) == 2
    assert sorted(os.listdir(ref_lib.REF_DIR)) == sorted([n + ".so" for n in NAMES] + ["manifest.json"])


def test_clean_checkout_without_the_reference_tree_records_why(tmp_path):
    out = tmp_path / "_ref"
    m = build_ref.build_ref(reference=str(tmp_path / "no_such_reference"), out_dir=str(out), verbose=False)
    assert m["built"] is False and "not found" in m["reason"]
    assert os.listdir(out) == ["manifest.json"] and json.load(open(out / "manifest.json")) == m
    assert build_ref.build_ref(reference=str(tmp_path / "no_such_reference"), out_dir=str(out)) == m  # and again
    with pytest.raises(pytest.skip.Exception, match="not found"):
        ref_lib.load("_ref_raymarching", ref_dir=str(out))


def test_a_broken_build_fails_instead_of_skipping(tmp_path):
    with pytest.raises(pytest.fail.Exception, match="missing"):
        ref_lib.load("_ref_chamfer", ref_dir=str(tmp_path))  # no manifest at all
    (tmp_path / "manifest.json").write_text(json.dumps({"built": True, "modules": {"_ref_chamfer": "_ref_chamfer.so"}}))
    with pytest.raises(pytest.fail.Exception, match="missing"):
        ref_lib.load("_ref_chamfer", ref_dir=str(tmp_path))  # says built, module absent
    (tmp_path / "_ref_chamfer.so").write_bytes(b"not a shared object")
    with pytest.raises(pytest.fail.Exception, match="does not import"):
        ref_lib.load("_ref_chamfer", ref_dir=str(tmp_path))


def test_binaries_that_travelled_without_the_reference_tree_are_kept(tmp_path):
    """On a machine without the reference tree (the GPU machine), build() must leave the binaries and the manifest it finds."""
    out = tmp_path / "_ref"
    out.mkdir()
    m = {"built": True, "modules": {n: n + ".so" for n in NAMES}, "sources": {}}
    (out / "manifest.json").write_text(json.dumps(m))
    for n in NAMES:
        (out / (n + ".so")).write_bytes(b"x")
    assert build_ref.build_ref(reference=str(tmp_path / "no_such_reference"), out_dir=str(out)) == m
    assert sorted(os.listdir(out)) == sorted([n + ".so" for n in NAMES] + ["manifest.json"])
    os.remove(out / "_ref_chamfer.so")  # incomplete: nothing to keep
    assert build_ref.build_ref(reference=str(tmp_path / "no_such_reference"), out_dir=str(out))["built"] is False
