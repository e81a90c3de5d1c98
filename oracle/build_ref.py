"""Recipe for oracle/_ref: the reference's own native operators, compiled for gfx950 as checkers (test infrastructure).

Where the reference tree is present, its five native sources (raymarching.cu / raymarching.h / bindings.cpp and chamfer3D.cu /
chamfer_cuda.cpp) are copied -- unmodified -- into a work directory, translated and compiled by torch.utils.cpp_extension.load
(which hipifies CUDA sources under ROCm), and the three resulting Python extension modules are kept:

    _ref_raymarching        device code with -ffp-contract=off: every operation rounded, as the HIP kernels and the C oracle do
    _ref_raymarching_fmad   the same sources with hipcc's default contraction (counterpart of liboracle_raymarching_fmad.so)
    _ref_chamfer            -ffp-contract=off

Only the three .so files and manifest.json stay in oracle/_ref (git-ignored): the copied and translated sources, the object files
and ninja's files are deleted after linking, so that no reference program text lies in the tree.  manifest.json is always written:
{"built": true, ...versions, source digests, flags, module files} or {"built": false, "reason": ...} where there is no reference
tree (a clean checkout elsewhere) -- tests/ref_lib.py turns the latter into a skip and everything else that is missing into a failure.
A second call with unchanged digests, flags and versions builds nothing.  A tree that carries built binaries to a machine without the
reference tree keeps them: they cannot be rebuilt there, and the manifest says what they were built from.  Consequence: in that case
nothing is checked -- neither the torch / HIP versions nor the source digests nor that the modules load -- so binaries left over from
an older reference or torch are used as they are (tests/ref_lib.py fails if one does not import); delete oracle/_ref to be rid of them.
"""
import hashlib
import json
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "_ref")
REFERENCE = os.environ.get("NVSF_REFERENCE", "/root/reference")
ARCH = "gfx950"

_RAYMARCHING = ("nvsf/nerf/raymarching/src/raymarching.cu", "nvsf/nerf/raymarching/src/raymarching.h", "nvsf/nerf/raymarching/src/bindings.cpp")
_CHAMFER = ("nvsf/nerf/chamfer3D/chamfer3D.cu", "nvsf/nerf/chamfer3D/chamfer_cuda.cpp")
# name -> (sources relative to the reference tree, extra device/host flags of the hipcc lines)
MODULES = {
    "_ref_raymarching": (_RAYMARCHING, ["-ffp-contract=off"]),
    "_ref_raymarching_fmad": (_RAYMARCHING, []),
    "_ref_chamfer": (_CHAMFER, ["-ffp-contract=off"]),
}
EXPORTS = {
    "_ref_raymarching": ("near_far_from_aabb", "sph_from_ray", "morton3D", "morton3D_invert", "packbits", "march_rays_train",
                         "composite_rays_train_forward", "composite_rays_train_backward", "march_rays", "composite_rays"),
    "_ref_chamfer": ("forward", "backward"),
}
EXPORTS["_ref_raymarching_fmad"] = EXPORTS["_ref_raymarching"]


def _write_manifest(out_dir, manifest):
    os.makedirs(out_dir, exist_ok=True)
    tmp = os.path.join(out_dir, "manifest.json.tmp")
    with open(tmp, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    os.replace(tmp, os.path.join(out_dir, "manifest.json"))
    return manifest


def _read_manifest(out_dir):
    try:
        with open(os.path.join(out_dir, "manifest.json")) as f:
            return json.load(f)
    except (OSError, ValueError):
        return None


def _complete(out_dir, manifest):
    return bool(manifest and manifest.get("built") and all(os.path.isfile(os.path.join(out_dir, f)) for f in manifest.get("modules", {}).values()))


def _jobs():
    try:
        return str(max(1, int(os.environ["MAX_JOBS"])))  # the caller's limit holds
    except (KeyError, ValueError):
        return "16"  # never sized by the machine's CPU count (two translation units per module anyway)


def _build_one(name, sources, flags, reference, out_dir, verbose):
    from torch.utils import cpp_extension
    work = os.path.join(out_dir, name)
    shutil.rmtree(work, ignore_errors=True)
    os.makedirs(work)
    try:
        local = []
        for rel in sources:
            dst = os.path.join(work, os.path.basename(rel))
            shutil.copyfile(os.path.join(reference, rel), dst)  # copyfile: contents only, so the copy is writable (hipify writes next to it)
            os.chmod(dst, 0o644)
            if not rel.endswith(".h"):
                local.append(dst)
        cpp_extension.load(name=name, sources=local, extra_cflags=["-O2"], extra_cuda_cflags=["-O2"] + flags,
                           build_directory=work, is_python_module=True, verbose=verbose)
        built = os.path.join(work, name + ".so")
        final = os.path.join(out_dir, name + ".so")
        os.replace(built, final)
        return os.path.basename(final)
    finally:
        shutil.rmtree(work, ignore_errors=True)  # copied + translated sources, objects, ninja files


def build_ref(reference=None, out_dir=None, verbose=False):
    """-> the manifest (dict) it wrote or found.  Raises only when a build that was attempted fails."""
    reference = REFERENCE if reference is None else reference
    out_dir = OUT_DIR if out_dir is None else out_dir
    old = _read_manifest(out_dir)
    wanted = sorted({rel for srcs, _ in MODULES.values() for rel in srcs})
    missing = [rel for rel in wanted if not os.path.isfile(os.path.join(reference, rel))]
    if missing:
        if _complete(out_dir, old):
            return old  # binaries that travelled here with the tree: kept as they are
        return _write_manifest(out_dir, {"built": False, "reason": f"reference sources not found under {reference} (first missing: {missing[0]})"})
    import torch
    if not getattr(torch.version, "hip", None):
        return _write_manifest(out_dir, {"built": False, "reason": "the installed torch is not a ROCm build"})
    digests = {}
    for rel in wanted:
        with open(os.path.join(reference, rel), "rb") as f:
            digests[rel] = hashlib.sha256(f.read()).hexdigest()
    manifest = {
        "built": True, "arch": ARCH, "torch": torch.__version__, "hip": torch.version.hip, "sources": digests,
        "flags": {name: flags for name, (_, flags) in MODULES.items()},
        "module_sources": {name: list(srcs) for name, (srcs, _) in MODULES.items()},
        "modules": {name: name + ".so" for name in MODULES},
    }
    if _complete(out_dir, old) and old == manifest:
        return old
    os.makedirs(out_dir, exist_ok=True)
    saved = {k: os.environ.get(k) for k in ("PYTORCH_ROCM_ARCH", "MAX_JOBS")}
    os.environ["PYTORCH_ROCM_ARCH"] = ARCH
    os.environ["MAX_JOBS"] = _jobs()
    try:
        for name, (srcs, flags) in MODULES.items():
            if verbose:
                print(f"oracle/_ref: building {name} {flags}", flush=True)
            _build_one(name, srcs, flags, reference, out_dir, verbose)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return _write_manifest(out_dir, manifest)


if __name__ == "__main__":
    m = build_ref(verbose="-v" in sys.argv)
    print(json.dumps({k: m[k] for k in ("built", "reason", "modules") if k in m}))
