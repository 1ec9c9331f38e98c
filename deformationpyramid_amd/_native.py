"""Loader and ctypes signatures for libndp_hip.so (the C ABI of include/ndp_hip.h).

There is deliberately NO fallback: if the HIP library is missing or an entry point fails, the
caller gets an exception.  `build()` compiles the library in-tree with hipcc for gfx950.
"""
import ctypes
import hashlib
import os
import re
import shutil
import subprocess

from .layout import CLayerDesc

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIBDIR = os.path.join(_HERE, "lib")
LIBPATH = os.path.join(LIBDIR, "libndp_hip.so")
SOURCES = ["ndp_kernels.hip"]                        # the one translation unit; what it includes is found by _closure()
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-pass-failed"]

NDP_MAX_LEVELS = 16
TILE = 64
NHMAX = 16
HROW = 24

c_float_p = ctypes.POINTER(ctypes.c_float)
c_int_p = ctypes.POINTER(ctypes.c_int)


class NdpError(RuntimeError):
    pass


class NdpUnservedError(NdpError, KeyError):
    """Registration.register() was asked for something this package does not serve: a `deformation_model` it has no path for, or
    any model on a CPU device (there is no CPU fallback).  One class for both, and both of its bases on purpose: callers that treat
    "not served here" as a failed lookup of the model (`except KeyError`, what an unknown model has always raised) and callers that
    catch the package's own NdpError keep working whichever of the two reasons applies."""

    def __str__(self):
        return RuntimeError.__str__(self)              # the message itself, not KeyError's repr of it


class PairGeom(ctypes.Structure):
    _fields_ = [("K", ctypes.c_int), ("S", ctypes.c_int), ("T", ctypes.c_int), ("pad", ctypes.c_int)]


class PairState(ctypes.Structure):
    _fields_ = [("level", ctypes.c_int), ("iter", ctypes.c_int), ("break_counter", ctypes.c_int),
                ("adam_t", ctypes.c_int), ("cur", ctypes.c_int), ("decision", ctypes.c_int),
                ("total_steps", ctypes.c_int), ("total_evals", ctypes.c_int), ("loss", ctypes.c_float),
                ("step_level", ctypes.c_int), ("step_t", ctypes.c_int), ("pad", ctypes.c_int),
                ("loss_prev", ctypes.c_double), ("evals_per_level", ctypes.c_int * NDP_MAX_LEVELS)]


# PairState.decision (the NDP_DEC_* enum of include/ndp_hip.h)
DEC_STEP, DEC_ADVANCE, DEC_STEP_ADVANCE, DEC_IDLE = 0, 1, 2, 3


class Engine(ctypes.Structure):
    _fields_ = [("desc", CLayerDesc), ("m", ctypes.c_int), ("k0", ctypes.c_int),
                ("P", ctypes.c_int), ("p_stride", ctypes.c_int),
                ("iters", ctypes.c_int), ("max_break_count", ctypes.c_int), ("early_stop", ctypes.c_int),
                ("B", ctypes.c_int), ("G", ctypes.c_int), ("n_cap", ctypes.c_int), ("t_cap", ctypes.c_int),
                ("break_threshold_ratio", ctypes.c_double),
                ("w_cd", ctypes.c_float), ("trunc", ctypes.c_float),
                ("adam_w1", ctypes.c_float), ("adam_b2", ctypes.c_float), ("adam_w2", ctypes.c_float),
                ("adam_eps", ctypes.c_float), ("w_reg", ctypes.c_float), ("pad_f", ctypes.c_float),
                ("geom", ctypes.c_void_p), ("state", ctypes.c_void_p), ("pts", ctypes.c_void_p),
                ("ldmk_t", ctypes.c_void_p), ("tgt", ctypes.c_void_p), ("params", ctypes.c_void_p),
                ("gpart", ctypes.c_void_p), ("adam_m", ctypes.c_void_p), ("adam_v", ctypes.c_void_p),
                ("act", ctypes.c_void_p), ("heads", ctypes.c_void_p),
                ("d2x", ctypes.c_void_p), ("idx_x", ctypes.c_void_p), ("d2y", ctypes.c_void_p),
                ("idx_y", ctypes.c_void_p), ("adam_tab", ctypes.c_void_p), ("dO", ctypes.c_void_p),
                ("nn_row", ctypes.c_void_p), ("nn_mode", ctypes.c_int), ("gemm_mode", ctypes.c_int),
                ("gmax", ctypes.c_void_p),
                ("nn_cells", ctypes.c_int), ("pad_i", ctypes.c_int),
                ("nnc_geom", ctypes.c_void_p), ("nnc_start", ctypes.c_void_p), ("nnc_rec", ctypes.c_void_p),
                ("nn_cells_wide", ctypes.c_int), ("pad_w", ctypes.c_int)]


class WarpJob(ctypes.Structure):
    _fields_ = [("params", ctypes.c_void_p), ("x", ctypes.c_void_p), ("x_out", ctypes.c_void_p),
                ("shift_in", ctypes.c_void_p), ("shift_out", ctypes.c_void_p), ("n", ctypes.c_int), ("pad", ctypes.c_int)]


class LoadJob(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("tgt", ctypes.c_void_p), ("perm_s", ctypes.c_void_p),
                ("perm_t", ctypes.c_void_p), ("ldmk_s", ctypes.c_void_p), ("ldmk_t", ctypes.c_void_p),
                ("params", ctypes.c_void_p), ("means", ctypes.c_void_p),
                ("slot", ctypes.c_int), ("K", ctypes.c_int), ("S", ctypes.c_int), ("T", ctypes.c_int),
                ("n_src", ctypes.c_int), ("n_tgt", ctypes.c_int)]


class StageLaunch(ctypes.Structure):
    """ndp_stage_launch: one launch of a tick as ndp_engine_plan reports it (extra: the kernel's third integer argument, or -1)."""
    _fields_ = [("kernel", ctypes.c_char_p), ("stage", ctypes.c_int), ("grid", ctypes.c_int * 3), ("block", ctypes.c_int),
                ("lds_bytes", ctypes.c_int), ("extra", ctypes.c_int)]


MAX_WARP_JOBS = 32
TICK_KERNELS = ("k_eng_fwd", "k_eng_nn", "k_eng_loss", "k_eng_bwd2", "k_eng_bwd1", "k_eng_update")   # one tick, launch order
MAX_LOAD_JOBS = 16
NNC_START = 4104                     # NDP_NNC_START: ints per cell_start table of the cell search
NNC_MAX, NNW_MAX = 2048, 8192        # points per cloud of the cell search (nn_cells) and of its wide form (nn_cells_wide)


def _closure(sources):
    """{path: bytes} of everything the compiler reads for `sources` (names under CSRC): the sources, then every `#include "..."` reached
    from them, resolved relative to the including file as the compiler does -- depth first in include order, each file once."""
    seen = {}
    def visit(path):
        path = os.path.normpath(path)
        if path not in seen:
            with open(path, "rb") as f:
                seen[path] = f.read()
            for inc in re.findall(rb'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', seen[path], re.M):
                visit(os.path.join(os.path.dirname(path), inc.decode()))
    for s in sources:
        visit(os.path.join(CSRC, s))
    return seen


def _tree_id(sources, flags):
    """Hex digest of _closure(sources) and of the compile flags, or None in a deployment without csrc/ (the prebuilt library's
    embedded id stands then, see _is_stale).  An #include that names no file is an error, not such a deployment."""
    if not os.path.exists(os.path.join(CSRC, sources[0])):
        return None
    h = hashlib.sha256()
    for text in _closure(sources).values():
        h.update(text)
    h.update(" ".join(flags).encode())
    return h.hexdigest()[:16]


def _built_id(path, tag=b"NDP_BUILD_ID"):
    """Build id of an existing library file (the tag string ndp_build_id() returns, found without loading it), or None."""
    try:
        with open(path, "rb") as f:
            hit = re.search(tag + rb"=([0-9a-f]{16})", f.read())
        return hit.group(1).decode() if hit else None
    except OSError:
        return None


def _is_stale(path, tag, tree_id):
    built = _built_id(path, tag)         # None: no such file, or it carries no id
    return built is None if tree_id is None else built != tree_id       # no sources to compare with: any library with an id is taken as built


def _build(path, tag, macro, sources, flags, compilers, lock, force, verbose=False):
    """Compile `sources` into `path` (in-tree) unless the id it carries is the tree's.  Serialised by a file lock with the staleness
    re-checked under it: N ranks that find a stale library build it once."""
    import fcntl
    tree_id = _tree_id(sources, flags)
    if not force and not _is_stale(path, tag, tree_id):
        return path
    os.makedirs(LIBDIR, exist_ok=True)
    with open(os.path.join(LIBDIR, lock), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if not force and not _is_stale(path, tag, tree_id):
            return path
        if tree_id is None:
            raise NdpError(f"{path} is missing (or carries no build id) and this deployment has no csrc/ to build it from: "
                           "ship the prebuilt library with the package (its layout is checked against the Python structs by ndp_abi_sizes)")
        cc = next((c for c in (shutil.which(compilers[0]),) + compilers[1:] if c and os.path.exists(c)), None)
        if cc is None:
            raise NdpError(f"{compilers[0]} not found and {os.path.basename(path)} is missing or stale")
        tmp = f"{path}.{os.getpid()}.tmp"             # build aside + atomic rename: nobody ever sees a torn file
        cmd = [cc] + flags + [f'-D{macro}="{tree_id}"', "-o", tmp] + [os.path.join(CSRC, s) for s in sources]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        os.replace(tmp, path)
    return path


def source_id():
    """Digest of everything libndp_hip.so is compiled from and of the compile flags, compiled into the library (-DNDP_BUILD_ID) and
    returned by ndp_build_id(): a library whose id differs from the tree's was built from other sources -- lib() rebuilds it or refuses
    to load it, because ndp_engine / ndp_load_job are passed BY VALUE into kernels and a stale layout would corrupt device memory."""
    return _tree_id(SOURCES, HIPCC_FLAGS)


# what SOURCES include, relative to CSRC ("ndp_device.h", "ndp_nn_cells.inc", "../../include/ndp_hip.h", ...): computed, for readers
HEADERS = [os.path.relpath(p, CSRC) for p in list(_closure(SOURCES))[len(SOURCES):]] if os.path.isdir(CSRC) else []


def _stale():
    return _is_stale(LIBPATH, b"NDP_BUILD_ID", source_id())


def build(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 ... -> deformationpyramid_amd/lib/libndp_hip.so (in-tree)."""
    return _build(LIBPATH, b"NDP_BUILD_ID", "NDP_BUILD_ID", SOURCES, HIPCC_FLAGS, ("hipcc", "/opt/rocm/bin/hipcc"), ".build.lock", force, verbose)


_LIB = None
V = ctypes.c_void_p
I = ctypes.c_int
F = ctypes.c_float
DP = ctypes.POINTER(CLayerDesc)

_SIGS = {
    "ndp_level_fwd": [DP, V, I, I, V, I, V, V, V, V, V],
    "ndp_level_bwd": [DP, V, I, I, V, I, V, V, V, V, V, V, I, I, V, V],
    "ndp_grad_reduce": [V, I, I, I, V, V],
    "ndp_pyramid_fwd": [DP, I, I, V, I, V, I, V, V],
    "ndp_pyramid_jac": [DP, I, I, V, I, I, I, V, I, V, V, V, V, V],
    "ndp_pyramid_inverse": [DP, I, I, V, I, I, I, V, I, V, I, F, V, V, V],
    "ndp_pyramid_fwd_batch": [DP, I, I, I, ctypes.POINTER(WarpJob), I, V],
    "ndp_pyramid_fwd_batch_split": [DP, I, I, I, ctypes.POINTER(WarpJob), I, V],
    "ndp_pyramid_fwd_batch_split_tiles": [DP, I, I, I, ctypes.POINTER(WarpJob), I, I, V],
    "ndp_pair_means": [V, I, V, I, V, V],
    "ndp_nsfp_fwd": [V, V, I, V, V, V, V],
    "ndp_nsfp_bwd": [V, V, I, V, V, V, V, I, I, V],
    "ndp_ed_warp": [V, I, V, V, V, I, V, V, V, V, V],
    "ndp_ed_arap": [V, I, V, V, V, V, I, V, V],
    "ndp_ed_grad": [V, I, V, V, V, V, I, V, V, V, V, V, I, F, V, V],
    "ndp_nerfies_fwd": [V, V, I, c_float_p, V, V, V, V, I, V, V, V, V],
    "ndp_nerfies_bwd": [V, V, I, V, V, V, V, V, V, I, I, V],
    "ndp_chamfer_nn_fwd": [V, I, V, I, V, V, V, V, V],
    "ndp_chamfer_nn_onepass": [V, I, V, I, V, V, V, V, V, V],
    "ndp_chamfer_nn_matrix": [V, I, V, I, V, V, V, V, V, V],
    "ndp_engine_nn_matrix_fits": [I],
    "ndp_engine_nn_onepass_fits": [I],
    "ndp_chamfer_nn_cells": [V, I, V, I, V, V, V, V, V, V, V, V],
    "ndp_chamfer_nn_cells_workspace": [I, ctypes.POINTER(ctypes.c_longlong)],
    "ndp_engine_nn_cells_fits": [I, I],
    "ndp_chamfer_nn_cells_wide": [V, I, V, I, V, V, V, V, V, V, V, V],
    "ndp_chamfer_nn_cells_wide_workspace": [I, I, ctypes.POINTER(ctypes.c_longlong)],
    "ndp_engine_nn_cells_wide_fits": [I, I],
    "ndp_chamfer_l1_bwd": [V, I, V, I, F, V, V, V, V, V, V, I, V],
    "ndp_flow_metrics": [V, V, V, I, V, V],
    "ndp_landmark_mse_fwd_bwd": [V, V, I, V, V, V],
    "ndp_adam_step": [V, V, V, V, I, F, F, F, F, F, F, V],
    "ndp_engine_run": [ctypes.POINTER(Engine), I, I, V],
    "ndp_engine_run_timed": [ctypes.POINTER(Engine), I, I, V, c_float_p],
    "ndp_engine_run_stages": [ctypes.POINTER(Engine), I, I, I, V],
    "ndp_engine_load": [ctypes.POINTER(Engine), I, ctypes.POINTER(LoadJob), I, V],
    "ndp_engine_plan": [ctypes.POINTER(Engine), ctypes.POINTER(StageLaunch), c_int_p],
    "ndp_sinkhorn_schedule": [ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.POINTER(ctypes.c_double), I],
    "ndp_sinkhorn_workspace": [I, I, ctypes.POINTER(ctypes.c_longlong)],
    "ndp_sinkhorn_divergence": [V, I, V, I, F, F, F, ctypes.c_double, V, V, V, V, V],
    "ndp_knn": [V, I, V, I, I, V, V, V],
    "ndp_normals_from_knn": [V, I, V, I, V, V, V, V],
    "ndp_point_to_plane": [V, I, V, I, V, V, F, V, V, V, V, I, V, V, V],
    "ndp_rigid_fit": [V, V, V, V, V, c_int_p, I, F, V, V, V, V, V],
    "ndp_rigid_score": [V, V, V, V, c_int_p, I, I, F, V, V, V],
    "ndp_ransac_rigid_workspace": [I, I, ctypes.POINTER(ctypes.c_longlong)],
    "ndp_ransac_rigid": [V, V, V, c_int_p, I, V, I, F, F, I, V, V, V, V, V, V, V, V, V, V, V, V],
    "ndp_feat_rowstats": [V, V, V, V, c_int_p, c_int_p, I, I, F, V, V, V, V, V, V],
    "ndp_feat_match_workspace": [I, ctypes.c_longlong, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)],
    "ndp_feat_match": [V, V, V, V, c_int_p, c_int_p, I, I, I, F, F, I, F, I, V, V, V, V],
    "ndp_voxel_subsample_workspace": [ctypes.c_longlong, I, ctypes.POINTER(ctypes.c_longlong)],
    "ndp_voxel_subsample": [V, V, I, c_int_p, I, F, I, V, ctypes.c_longlong, V, V, V, c_int_p, V],
    "ndp_radius_search_workspace": [ctypes.c_longlong, ctypes.c_longlong, I, ctypes.POINTER(ctypes.c_longlong)],
    "ndp_radius_search": [V, V, c_int_p, c_int_p, I, F, I, V, ctypes.c_longlong, V, V, V, V],
    "ndp_kpconv_forward_workspace": [ctypes.c_longlong, ctypes.c_longlong, I, I, I, I, ctypes.POINTER(ctypes.c_longlong)],
    "ndp_kpconv_forward": [V, V, V, V, V, V, ctypes.c_longlong, ctypes.c_longlong, I, I, I, I, F, I, I, I, V, ctypes.c_longlong, V, V],
    "ndp_kpconv_backward_workspace": [ctypes.c_longlong, ctypes.c_longlong, I, I, I, I, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)],
    "ndp_kpconv_backward": [V, V, V, V, V, V, V, ctypes.c_longlong, ctypes.c_longlong, I, I, I, I, F, I, I, I, ctypes.c_longlong, V,
                            ctypes.c_longlong, V, V, V],
    "ndp_attention_forward": [V, V, V, V, V, V, V, c_int_p, c_int_p, I, I, I, F, V, V],
    "ndp_attention_compat_forward": [V, V, V, V, V, V, V, V, V, c_int_p, c_int_p, I, I, I, F, ctypes.c_double, V, V],
    "ndp_feat_conf_workspace": [I, ctypes.c_longlong, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)],
    "ndp_feat_conf": [V, V, V, V, c_int_p, c_int_p, I, I, F, V, V, I, I, V],
    "ndp_attention_forward_lse": [V, V, V, V, V, V, V, V, V, c_int_p, c_int_p, I, I, I, F, ctypes.c_double, V, V, V],
    "ndp_attention_backward": [V, V, V, V, V, V, V, V, V, V, V, V, c_int_p, c_int_p, I, I, I, F, ctypes.c_double, V, V, V, V, V],
}
ABI_VERSION = 215                                   # the ABI this signature table was last renumbered at; entries added since (216:
                                                    # ndp_attention_compat_forward; 217: ndp_attention_forward_lse, ndp_attention_backward;
                                                    # 218: ndp_engine_plan; 219: ndp_kpconv_backward_workspace, ndp_kpconv_backward,
                                                    # next to the forward's as ndp_engine_plan is next to the engine's)
                                                    # only append, and ndp_version() tells what a library has
EXPORTS = ["ndp_version", "ndp_last_error", "ndp_build_id", "ndp_abi_sizes", "ndp_engine_nn_workspace"] + list(_SIGS)


_VARIANT = None


def use_variant(path):
    """Measurement tools only (tools/_modes.py): load `path` -- a timing / experiment build of libndp_hip.so -- instead of the
    product library, before anything else touched it.  Explicit by construction: no environment variable reaches this, the build-id
    check is the caller's to give up, and `variant()` lets bench.py record (and refuse) it."""
    global _VARIANT
    if _LIB is not None:
        raise NdpError("use_variant() after the library was loaded")
    _VARIANT = os.path.abspath(path)


def variant():
    return _VARIANT


def lib(allow_build=True):
    """Load the native library (building it first if the source is newer and hipcc exists)."""
    global _LIB
    if _LIB is None:
        # The library carries the digest of the sources it was built from (ndp_build_id): an absent or stale library is
        # rebuilt (under a file lock, so N ranks build once), and one that cannot be rebuilt is refused -- never loaded.
        override = _VARIANT                          # set by use_variant() only: the package reads no environment variable
        if not override:
            have_hipcc = bool(shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"))
            if allow_build and have_hipcc and _stale():
                build()
            if not os.path.exists(LIBPATH):
                raise NdpError(f"{LIBPATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
            if source_id() is not None and _built_id(LIBPATH) != source_id():
                raise NdpError(f"{LIBPATH} was built from other sources (build id {_built_id(LIBPATH)}, tree {source_id()}): "
                               "run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = ctypes.CDLL(override or LIBPATH)
        L.ndp_version.restype = I
        L.ndp_last_error.restype = ctypes.c_char_p
        L.ndp_build_id.restype = ctypes.c_char_p
        L.ndp_abi_sizes.argtypes = [c_int_p]
        L.ndp_abi_sizes.restype = I
        L.ndp_engine_nn_workspace.argtypes = [I, I, ctypes.POINTER(ctypes.c_longlong)]
        L.ndp_engine_nn_workspace.restype = I
        sizes = (ctypes.c_int * 6)()
        L.ndp_abi_sizes(sizes)
        mine = [ctypes.sizeof(t) for t in (CLayerDesc, PairGeom, PairState, Engine, WarpJob, LoadJob)]
        if list(sizes) != mine:
            raise NdpError(f"struct layouts differ between {override or LIBPATH} {list(sizes)} and the ctypes mirror {mine}")
        for name, args in _SIGS.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = I
        _LIB = L
    return _LIB


# ------------------------------------------------------------------ host runtime library (no GPU)
HOST_LIBPATH = os.path.join(LIBDIR, "libndp_host.so")
HOST_SOURCES = ["ndp_host.cpp", "ndp_graph.cpp"]                          # RNG replay; embedded-deformation graph builder
HOST_FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-mfma", "-mavx2", "-fPIC", "-shared"]
_HOST = None


class DrawOp(ctypes.Structure):
    _fields_ = [("n", ctypes.c_longlong), ("lo", ctypes.c_float), ("hi", ctypes.c_float), ("offset", ctypes.c_longlong)]


def _host_id():
    """Digest of the host library's sources and flags (compiled in as NDP_HOST_BUILD_ID), or None without sources."""
    return _tree_id(HOST_SOURCES, HOST_FLAGS)


def build_host(force=False):
    """g++ -> deformationpyramid_amd/lib/libndp_host.so; rebuilt when the digest of its sources changes."""
    return _build(HOST_LIBPATH, b"NDP_HOST_ID", "NDP_HOST_BUILD_ID", HOST_SOURCES, HOST_FLAGS, ("g++",), ".build_host.lock", force)


def host_lib():
    global _HOST
    if _HOST is None:
        if shutil.which("g++") and _host_id() is not None:
            build_host()                                # no-op when the embedded digest matches
        if not os.path.exists(HOST_LIBPATH):
            raise NdpError(f"{HOST_LIBPATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        if _is_stale(HOST_LIBPATH, b"NDP_HOST_ID", _host_id()):     # cannot be rebuilt here (no g++): refuse it, like the HIP library
            raise NdpError(f"{HOST_LIBPATH} was built from other sources (build id {_built_id(HOST_LIBPATH, b'NDP_HOST_ID')}, "
                           f"tree {_host_id()}): run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = ctypes.CDLL(HOST_LIBPATH)
        L.ndp_rng_replay.argtypes = [V, ctypes.c_longlong, ctypes.POINTER(DrawOp), I, I, V, ctypes.c_longlong]
        L.ndp_rng_replay.restype = I
        L.ndp_rng_skip.argtypes = [V, ctypes.c_longlong, ctypes.c_longlong]
        L.ndp_rng_skip.restype = I
        L.ndp_pair_draws.argtypes = [ctypes.POINTER(DrawOp), I, I, I]
        L.ndp_pair_draws.restype = ctypes.c_longlong
        L.ndp_pair_init.argtypes = [V, ctypes.c_longlong, ctypes.POINTER(DrawOp), I, V, I, I, I, V, V, V]
        L.ndp_pair_init.restype = I
        L.ndp_host_build_id.restype = ctypes.c_char_p
        L.ndp_depth_to_mesh.argtypes = [V, I, I, F, V, V, V, c_int_p, c_int_p]
        L.ndp_erode_mesh.argtypes = [I, V, I, I, I, V]
        L.ndp_sample_nodes.argtypes = [V, I, V, F, I, V]
        L.ndp_edges_geodesic.argtypes = [V, I, V, V, I, V, I, I, F, I, I, V, V, V]
        L.ndp_edges_geodesic.restype = V
        L.ndp_geodesic_free.argtypes = [V]
        L.ndp_geodesic_free.restype = None
        L.ndp_node_cleanup.argtypes = [V, I, I, V]
        L.ndp_pixel_anchors.argtypes = [V, V, V, I, I, I, F, V, V]
        for name in ("ndp_depth_to_mesh", "ndp_erode_mesh", "ndp_sample_nodes", "ndp_node_cleanup", "ndp_pixel_anchors"):
            getattr(L, name).restype = I
        _HOST = L
    return _HOST


def make_draw_ops(ops):
    return (DrawOp * len(ops))(*[DrawOp(int(n), float(lo), float(hi), int(off)) for n, lo, hi, off in ops])


def rng_replay(ops, out):
    """Run draw ops on torch's global CPU generator (state exported, advanced natively, re-imported)."""
    import torch
    if not isinstance(ops, ctypes.Array):
        ops = make_draw_ops(ops)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.device.type == "cpu"
    st = torch.get_rng_state()
    rc = host_lib().ndp_rng_replay(ctypes.c_void_p(st.data_ptr()), st.numel(), ops, len(ops), 1,
                                   ctypes.c_void_p(out.data_ptr()), 0)
    if rc != 0:
        raise NdpError("ndp_rng_replay failed")
    torch.set_rng_state(st)


def check(rc, what):
    if rc != 0:
        msg = lib().ndp_last_error().decode(errors="replace")
        raise NdpError(f"{what} failed (rc={rc}): {msg}")


def stream_ptr(device=None):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
