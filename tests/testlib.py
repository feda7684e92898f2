"""Helpers shared by the CPU and GPU test tiers."""
import ctypes
import glob
import hashlib
import os
import re
import subprocess
import tempfile

import numpy as np

from svsdct import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(REPO, "secure-video-steganography-using-ecc-and-dct_amd")
CSRC = os.path.join(PKG_DIR, "csrc")
EXP_LIB_PATH = os.path.join(PKG_DIR, "lib", "variants", "libsvsdct_exp.so")

# measurement hooks: exported by the EXPERIMENTS library only (csrc/svs_capi.hip, -DSVS_EXPERIMENTS)
EXPERIMENT_HOOKS = {
    "svs_guard_counter_set": (ctypes.c_int, [ctypes.c_void_p]),
    "svs_ref_copy_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]),
    "svs_ref_read_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "svs_probe_cvt_pk_u8": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
}
_exp_lib = None


def experiments_library():
    """lib/variants/libsvsdct_exp.so with every prototype of the product ABI plus the measurement hooks attached.  Built by
    __graft_entry__.build(); the same kernel sources as the product library, so it has to pass the golden vectors itself
    (tests/test_gpu_parity.py::test_experiments_library_reproduces_the_golden_vectors)."""
    global _exp_lib
    if _exp_lib is None:
        from svsdct import native
        if not os.path.exists(EXP_LIB_PATH):       # normally built by __graft_entry__.build(); hipcc is in the image (about 25 s)
            try:
                subprocess.run(["make", "-C", CSRC, "exp"], check=True, capture_output=True, timeout=600)
            except (OSError, subprocess.SubprocessError) as exc:
                raise RuntimeError(f"{EXP_LIB_PATH} is missing and could not be built ({exc}): run `python __graft_entry__.py`") from exc
        lib = ctypes.CDLL(EXP_LIB_PATH)
        for name, (res, args) in {**native.SIGNATURES, **EXPERIMENT_HOOKS}.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _exp_lib = lib
    return _exp_lib


class using_library:
    """`with using_library(experiments_library()):` - svsdct.batch / native route their calls to that library inside the block"""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        from svsdct import native
        self.saved, native._lib = native._lib, self.lib
        return self.lib

    def __exit__(self, *exc):
        from svsdct import native
        native._lib = self.saved
        return False


def natural_like(h, w, seed):
    """A frame with what real video has and uniform noise lacks: flat black bars, saturated highlights, smooth gradients,
    low-amplitude texture - the content on which the reference's round-trip artefacts and clipping show."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = 128 + 90 * np.sin(xx / 97.0) * np.cos(yy / 61.0) + rng.normal(0, 2.0, (h, w))
    img[: h // 8] = 0                      # letterbox
    img[-h // 8:] = 16
    img[h // 3: h // 2, w // 4: w // 2] = 255          # blown-out highlight
    img[h // 2: h // 2 + 64, : w // 3] = 128            # flat mid-gray panel
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def structured_covers(h, w, seed=0):
    """name -> gray frame with structure that makes MANY blocks' coefficient changes structurally zero or integer-valued
    (VERDICT r01 'What's weak' #1): there the reference's output is decided by pocketfft's round-trip noise.  The second
    half of the list are the content classes of the round-2 review's adversarial probe."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    text = np.repeat(np.repeat(rng.integers(0, 2, (h // 4 + 1, w // 4 + 1), dtype=np.uint8), 4, axis=0), 4, axis=1)[:h, :w]
    abba = np.array([40, 200, 200, 40], np.uint8)[(np.arange(w) % 4)]
    # blocks base + outer(r, c) with sum r = sum c = 0: every row-0 / column-0 AC coefficient vanishes by exact cancellation
    outer = np.empty((h, w), np.int64)
    for by in range(h // 8):
        for bx in range(w // 8):
            r = rng.integers(-5, 6, 8); r[7] -= r.sum()
            c = rng.integers(-5, 6, 8); c[7] -= c.sum()
            outer[8 * by: 8 * by + 8, 8 * bx: 8 * bx + 8] = 128 + np.clip(np.outer(r, c), -100, 100)
    return {
        "natural_like": natural_like(h, w, seed + 1),
        "flat_128": np.full((h, w), 128, np.uint8),
        "constant_rows": np.repeat(rng.integers(16, 240, (h, 1), dtype=np.uint8), w, axis=1),   # vertical structure only
        "constant_columns": np.repeat(rng.integers(16, 240, (1, w), dtype=np.uint8), h, axis=0),
        "half_letterbox": np.concatenate([np.full((h // 2, w), 16, np.uint8),
                                          rng.integers(16, 240, (h - h // 2, w), dtype=np.uint8)]),
        "checker_8": ((np.add.outer(np.arange(h) // 8, np.arange(w) // 8) % 2) * 200 + 20).astype(np.uint8),
        "ramp": np.repeat((np.arange(w) // 4 % 256).astype(np.uint8)[None], h, axis=0),
        "dark_noise_0_3": rng.integers(0, 4, (h, w), dtype=np.uint8),
        "bright_noise_252_255": rng.integers(252, 256, (h, w), dtype=np.uint8),
        "posterised_sinusoid": (np.round((128 + 100 * np.sin(xx / 23.0) * np.cos(yy / 17.0)) / 32) * 32).clip(0, 255).astype(np.uint8),
        "text_4x4_binary": (text * 255).astype(np.uint8),
        "abba_stripes": np.repeat(abba[None], h, axis=0),
        "lsb_noise_on_flat": (100 + rng.integers(0, 2, (h, w))).astype(np.uint8),
        "outer_product_blocks": outer.clip(0, 255).astype(np.uint8),
        # smooth content: every block of a ramp has the SAME AC coefficients, a zero-heavy payload
        # requantises them to 0 and the block comes out flat at its mean - on the integer grid in 1 block of 8
        "horizontal_ramp": np.clip(np.rint(xx * 255.0 / (w - 1)), 0, 255).astype(np.uint8),
        "vertical_ramp": np.clip(np.rint(yy * 255.0 / (h - 1)), 0, 255).astype(np.uint8),
        "diagonal_ramp": np.clip(np.rint((xx + yy) * 255.0 / (w + h - 2)), 0, 255).astype(np.uint8),
        "slow_sinusoid": np.clip(np.rint(128 + 90 * np.sin(xx / 97.0) * np.cos(yy / 61.0)), 0, 255).astype(np.uint8),
        "gaussian_sigma1_on_128": np.clip(np.rint(128 + rng.normal(0, 1.0, (h, w))), 0, 255).astype(np.uint8),
        "near_black_0_1": rng.integers(0, 2, (h, w), dtype=np.uint8),
    }


SMOOTH_COVERS = ("horizontal_ramp", "vertical_ramp", "diagonal_ramp", "slow_sinusoid", "gaussian_sigma1_on_128", "near_black_0_1")


def contract_payloads(n_bits, seed):
    """name -> payload of the FAST contract checks: Bernoulli(1/2) - under which 'all of a block's bits are 0' has
    probability 2^-n and is never seen at n >= 8 -, all zero, and 1 % ones: the reference's real stream opens with a
    976-bit header full of zero bytes (embed_process.py:62-74), and a block whose bits are all 0 has every near-zero
    coefficient requantised to exactly 0."""
    rng = np.random.default_rng(seed)
    return {"bernoulli_half": synth.synthetic_bits(n_bits, seed=seed),
            "all_zero": np.zeros(n_bits, np.uint8),
            "one_percent_ones": (rng.random(n_bits) < 0.01).astype(np.uint8)}


ORIGINAL_COVERS = ("natural_like", "flat_128", "constant_rows", "constant_columns", "half_letterbox", "checker_8", "ramp")

# (n_ac, delta) points of the FAST-mode contract checks on structured content plus the settings at
# which the index-4 / two-row coincidences are largest; (1, 8), (16, 8), (36, 8), (63, 4) added after VERDICT r02 next #3
CONTRACT_POINTS = [(3, 8), (3, 16), (7, 4), (10, 20), (4, 8), (8, 4), (8, 2), (1, 8), (16, 8), (36, 8), (63, 4), (9, 8),
                   # large steps at n >= 8 (the GUI offers delta 1..100, app.py:232)
                   (8, 20), (10, 64), (11, 64), (15, 100), (16, 64), (63, 64)]
# (n_ac, delta) points of the GUARDED-mode identity checks (one and two coefficient rows; the ends of the delta range included)
GUARDED_POINTS = [(3, 8), (1, 8), (7, 4), (4, 8), (3, 16), (5, 0.5), (2, 0.25), (3, 100), (7, 4096), (6, 7.3),
                  (10, 8), (8, 4), (15, 20), (12, 0.5), (9, 100), (10, 4096)]


def psnr_gap(a, b):
    """|a - b| in dB; 0 when both are infinite (stego == cover in both: nothing was changed)"""
    if np.isinf(a) or np.isinf(b):
        return 0.0 if a == b else float("inf")
    return abs(a - b)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def single_frame_cases(meta):
    return [k for k in meta["cases"] if k != "G8_stream"]


def case_inputs(arrays, meta, name):
    """-> (info, gray uint8[H,W], payload 0/1 array (possibly empty))"""
    info = meta["cases"][name]
    if name + "/gray" in arrays.files:
        gray = arrays[name + "/gray"]
    else:
        h, w = info["shape"]
        gray = synth.synthetic_frames(1, h, w, seed=info["synth_seed"])[0]
    if info["payload_len"] is None:
        payload = np.zeros(0, np.uint8)
    elif name + "/payload" in arrays.files:
        payload = arrays[name + "/payload"]
    else:
        payload = synth.synthetic_bits(info["payload_len"], seed=info["synth_seed"])
    return info, gray, payload


def golden_bits(arrays, name, tag, n_bits):
    return np.unpackbits(arrays[f"{name}/{tag}"], count=n_bits) if n_bits else np.zeros(0, np.uint8)


def exact_tie_mask(gray, delta, n_ac):
    """Boolean [blocks, n] mask of coefficients whose value c/delta is EXACTLY k+1/2.

    For integer pixels the coefficients at flat indices 4, 32, 36 are exact multiples of 1/8
    (their basis is +-1/8), so c/delta can land exactly on a rounding tie; which way the
    reference rounds then depends on pocketfft's float32 rounding noise.  Computed
    in exact integer arithmetic; integer delta only."""
    n = max(0, min(int(n_ac), 63))
    h, w = gray.shape
    blocks = gray.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8).astype(np.int64)
    s4 = np.array([1, -1, -1, 1, 1, -1, -1, 1], np.int64)
    mask = np.zeros((blocks.shape[0], n), bool)
    if delta <= 0 or int(delta) != delta:
        return mask
    d = int(delta)
    m = {4: (blocks.sum(1) * s4).sum(1), 32: (blocks.sum(2) * s4).sum(1),
         36: np.einsum("byx,y,x->b", blocks, s4, s4)}
    for k, val in m.items():
        if k <= n:
            mask[:, k - 1] = (val - 4 * d) % (8 * d) == 0
    return mask


# ---- test-only CPU build of the csrc/ headers (tests/hostemu): the only host C++ the tests build or load -----------------
_EMU = None
_C = ctypes
_PTR = ctypes.c_void_p


class EmuCall(ctypes.Structure):
    """tests/hostemu/emu_call.h, field for field"""
    _fields_ = [("size", _C.c_uint64), ("frames_in", _PTR), ("frames_out", _PTR), ("F", _C.c_int32), ("H", _C.c_int32),
                ("W", _C.c_int32), ("n_ac", _C.c_int32), ("delta", _C.c_double), ("index", _PTR), ("count", _C.c_int32),
                ("pocketfft", _C.c_int32), ("guarded", _C.c_int32), ("bits", _PTR), ("bits_bytes", _C.c_uint64),
                ("bit_offset", _C.c_uint64), ("n_bits", _C.c_uint64), ("nearest", _C.c_int32), ("minmove", _C.c_int32),
                ("dither", _C.c_int32), ("order", _C.c_int32), ("dither_key", _C.c_uint64), ("order_key", _C.c_uint64),
                ("first_frame", _C.c_uint32), ("guard_scale", _C.c_float), ("tie_scale", _C.c_float), ("force_qm", _C.c_int32),
                ("exact_rows", _C.c_int32), ("streaming_bodies", _C.c_int32), ("variant", _C.c_int32),
                ("extract_wave", _C.c_int32), ("keyed_form", _C.c_int32), ("output", _C.c_int32), ("vote_period", _C.c_uint64),
                ("vote_bit0", _C.c_uint64), ("replay_map", _PTR), ("candidate_map", _PTR), ("status", _PTR), ("bits_out", _PTR),
                ("soft_out", _PTR), ("tally", _PTR), ("hist", _PTR)]


class EmuResult(ctypes.Structure):
    _fields_ = [("size", _C.c_uint64), ("used", _C.c_uint64), ("replayed", _C.c_uint64), ("repaired", _C.c_uint64),
                ("unrepaired", _C.c_uint64), ("path", _C.c_int32), ("rows", _C.c_int32), ("qm", _C.c_int32),
                ("selected", _C.c_int32), ("dithered", _C.c_int32), ("nearest", _C.c_int32), ("minmove", _C.c_int32),
                ("word", _C.c_uint32), ("soft", _C.c_int32), ("vote", _C.c_int32), ("hist", _C.c_int32), ("keyed", _C.c_int32)]


EMU_BITS, EMU_SOFT, EMU_VOTE, EMU_HIST = range(4)      # EmuCall.output (emu_call.h EmuOutput)


_PROTOTYPES = {
    "emu_embed_call": (_C.c_int, [_C.POINTER(EmuCall), _C.POINTER(EmuResult)]),
    "emu_extract_call": (_C.c_int, [_C.POINTER(EmuCall), _C.POINTER(EmuResult)]),
    "emu_readback_call": (_C.c_int, [_C.POINTER(EmuCall), _C.POINTER(EmuResult)]),
    "emu_exact_mode": (None, [_C.POINTER(EmuCall), _C.c_int]),
    "emu_embed": (_C.c_uint64, [_PTR, _PTR, _C.c_int, _C.c_int, _C.c_int, _C.c_double, _C.c_int, _PTR, _C.c_uint64, _C.c_uint64,
                                _C.c_uint64, _C.c_int, _C.POINTER(_C.c_uint64)]),
    "emu_extract": (_C.c_uint64, [_PTR, _C.c_int, _C.c_int, _C.c_int, _C.c_double, _C.c_int, _PTR, _C.c_int,
                                  _C.POINTER(_C.c_uint64)]),
    "emu_pf_dct2": (None, [_PTR, _PTR]),
    "emu_pf_dct3": (None, [_PTR, _PTR]),
    "emu_forward_block": (None, [_PTR, _PTR]),
    "emu_idct8": (None, [_PTR, _PTR]),
    "emu_vertical_pf01": (None, [_PTR, _PTR]),
    "emu_qim_change_mismatches": (_C.c_uint64, [_PTR, _PTR, _C.c_uint64, _C.c_double]),
    "emu_quant_mismatches": (_C.c_uint64, [_PTR, _C.c_uint64, _C.c_double]),
    "emu_plan_chunks": (_C.c_uint64, [_C.c_int32, _C.c_int32, _C.c_uint64, _C.c_uint64, _C.c_uint64, _PTR, _C.c_uint64]),
    "emu_chunk_budget": (_C.c_uint64, [_C.c_uint64, _C.c_uint64, _C.c_uint64, _C.c_uint32]),
    "emu_plan_rule": (None, [_C.c_double, _C.c_int, _C.c_uint64, _C.c_uint64, _C.c_int, _C.c_int, _C.c_int, _C.c_int, _PTR]),
    "mm_margin": (_C.c_float, [_C.c_int]),
    "mm_coefficient": (None, [_C.c_float, _C.c_int, _C.c_double, _C.c_int, _C.c_int, _PTR]),
    "cs_table": (_C.c_int, [_PTR, _C.c_int, _PTR]),
    "dt_hash": (_C.c_float, [_C.c_uint64, _C.c_uint32, _C.c_uint32, _C.c_uint32, _C.c_float, _PTR]),
    "bo_map": (None, [_C.c_uint64, _C.c_uint32, _C.c_uint32, _C.c_uint32, _C.c_int, _PTR]),
    "bo_lowbias32": (_C.c_uint32, [_C.c_uint32]),
    "kc_apply": (None, [_PTR, _PTR, _PTR, _C.c_uint64, _PTR]),
    "kc_check": (_C.c_uint64, [_C.c_uint32, _C.c_uint32, _C.c_uint32, _C.c_int, _PTR, _PTR]),
    "emu_soft_args": (_C.c_int, [_C.POINTER(EmuCall), _PTR]),
    "emu_vote_residues": (_C.c_int, [_C.POINTER(EmuCall), _PTR, _C.c_uint64, _PTR, _PTR]),
    "emu_vote_of": (_C.c_int32, [_C.c_uint32, _C.c_int]),
    "emu_vote_period_max": (_C.c_uint64, []),
    "emu_hist_bins": (_C.c_uint32, []),
    "emu_hist_runs": (_C.c_uint32, [_C.c_uint32] * 5 + [_PTR, _C.c_uint32]),
}


HOSTEMU_DIR = os.path.join(REPO, "tests", "hostemu")
_BUILT = {}


def build_emu(source, prototypes, build_dir=None, extra_flags=()):
    """tests/hostemu/<source> (fec_emu.cpp -> libsvs_fec_emu.so) compiled with g++ against csrc/ into build_dir - a temporary
    directory when there is none; a CPU test passes its own and so compiles the file itself - and loaded, once per process, with
    prototypes = {name: (restype, argtypes)} attached.  extra_flags: -ffp-contract=off for an emulation of float code."""
    if source not in _BUILT:
        stem = os.path.splitext(source)[0]
        out = os.path.join(str(build_dir) if build_dir is not None else tempfile.mkdtemp(prefix=stem + "_"), f"libsvs_{stem}.so")
        subprocess.check_call(["g++", "-O2", *extra_flags, "-std=c++17", "-shared", "-fPIC", "-w", "-I" + CSRC,
                               os.path.join(HOSTEMU_DIR, source), "-o", out])
        lib = ctypes.CDLL(out)
        for name, (res, args) in prototypes.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _BUILT[source] = lib
    return _BUILT[source]


def run_sanitized_emu(source, define, tmp_path, says, extra_flags=()):
    """tests/hostemu/<source> with its own main (-D<define>) as a stand-alone program under the address and undefined-behaviour
    sanitizers, run once; it must end with status 0 and print `says`.  Nothing is loaded into python."""
    exe = str(tmp_path / (os.path.splitext(source)[0] + "_main"))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *extra_flags, "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D" + define, "-I" + CSRC, os.path.join(HOSTEMU_DIR, source), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and says in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])


def declared_symbols(header):
    """the svs_* functions that include/<header> declares, sorted"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(svs_[a-z0-9_]+)\s*\(", text)))


def nm_dynamic(lib_path, which="defined"):
    """the text of nm -D --defined-only (or which="undefined": --undefined-only) of a shared library"""
    return subprocess.run(["nm", "-D", f"--{which}-only", lib_path], capture_output=True, text=True, check=True).stdout


def exported_symbols(lib_path):
    """the svs_* symbols a shared library defines, sorted"""
    return sorted(line.split()[-1] for line in nm_dynamic(lib_path).splitlines() if line.split()[-1].startswith("svs_"))


def check_library_exports(header, binding, prefix, count, hidden=()):
    """include/<header> declares, the binding module's library exports and its SIGNATURES name the same `count` svs_* symbols; the
    library reports the binding's ABI version (<prefix>_abi_version), holds no dynamic symbol with one of `hidden` in its name,
    imports a kernel launch (nm really listed imports) and no getenv (it reads no environment variable).  -> the imports' text"""
    exported = exported_symbols(binding.LIB_PATH)
    assert exported == declared_symbols(header) == sorted(binding.SIGNATURES) and len(exported) == count
    defined = nm_dynamic(binding.LIB_PATH)
    assert not [line for line in defined.splitlines() if any(name in line for name in hidden)], defined
    assert getattr(binding.load(), prefix + "_abi_version")() == binding.ABI_VERSION
    undefined = nm_dynamic(binding.LIB_PATH, "undefined")
    assert "hipLaunchKernel" in undefined or "__hipPushCallConfiguration" in undefined
    assert "getenv" not in undefined
    return undefined


def check_header_is_plain_c(tmp_path, headers, expression):
    """a C99 program that includes `headers` in that order and returns 0 where `expression` holds: no warning, status 0"""
    src = tmp_path / "use.c"
    src.write_text("".join(f'#include "{h}"\n' for h in headers) + f"int main(void) {{ return {expression} ? 0 : 1; }}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(REPO, "include"), str(src), "-o",
                           str(tmp_path / "use")])
    subprocess.check_call([str(tmp_path / "use")])


def hostemu():
    global _EMU
    if _EMU is not None:
        return _EMU
    here = os.path.join(REPO, "tests", "hostemu")
    src, out = os.path.join(here, "hostemu.cpp"), os.path.join(here, "libsvs_hostemu.so")
    deps = glob.glob(os.path.join(CSRC, "*.hpp")) + [d for d in glob.glob(os.path.join(here, "*")) if d != out]
    stale = not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)
    if stale and os.path.exists(out) and os.path.exists("/dev/kfd"):
        stale = False      # on a GPU box use the library built by build(): no compiler child processes there
    if stale:
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-w",
                               "-I" + CSRC, src, "-o", out])
    lib = ctypes.CDLL(out)
    for name, (res, args) in _PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _EMU = lib
    return lib


def plan_chunks(n_frames, height, row_bytes, total_bytes=None, target_bytes=0):
    """the chunk plan of the host-pointer entry points (csrc/svs_stage.hpp) -> list of (f0, nf, r0, rows)"""
    lib = hostemu()
    total = n_frames * height * row_bytes if total_bytes is None else total_bytes
    n = lib.emu_plan_chunks(n_frames, height, row_bytes, total, target_bytes, None, 0)
    out = np.zeros((max(n, 1), 4), np.int32)
    assert lib.emu_plan_chunks(n_frames, height, row_bytes, total, target_bytes, out.ctypes.data, n) == n
    return [tuple(int(v) for v in row) for row in out[:n]]


def _fill_call(shape, delta, n_ac, bits=None, bit_offset=0, n_bits=None, index=None, exact=None, pocketfft=False,
               guarded=False, dither_key=None, block_key=None, **fields):
    """An EmuCall from NumPy arguments -> (the call, the arrays made here that it points into).  shape: (F, H, W) of its frames.
    bits: 0/1 per bit, packed here MSB-first and padded to whole dwords plus one; n_bits None: all of them from bit_offset on.
    index: None, or the flat indices of a coefficient selection.  exact: hostemu's mode number (emu_exact_mode) instead of the
    two mode bits.  dither_key / block_key: None, or the key of the dither / the block order.  fields: the remaining members of
    EmuCall by name (arrays by their address)."""
    lib = hostemu()
    f, h, w = shape
    keep = []          # the arrays made here that the call points into
    call = EmuCall(size=ctypes.sizeof(EmuCall), F=f, H=h, W=w, delta=float(delta), n_ac=int(n_ac), pocketfft=int(pocketfft),
                   guarded=int(guarded), guard_scale=1.0, tie_scale=1.0, force_qm=-1, exact_rows=8, streaming_bodies=1,
                   dither=int(dither_key is not None), dither_key=int(dither_key or 0), order=int(block_key is not None),
                   order_key=int(block_key or 0))
    if exact is not None:
        lib.emu_exact_mode(ctypes.byref(call), int(exact))
    if bits is not None:
        bits = np.asarray(bits, np.uint8)
        packed = np.packbits(bits)
        packed = np.concatenate([packed, np.zeros((-packed.size) % 4 + 4, np.uint8)])
        keep.append(packed)
        call.bits, call.bits_bytes, call.bit_offset = packed.ctypes.data, packed.size, int(bit_offset)
        call.n_bits = int(bits.size - bit_offset if n_bits is None else n_bits)
    if index is not None:
        idx = np.ascontiguousarray(np.asarray(index, np.int64).reshape(-1).astype(np.uint8))
        keep.append(idx)
        call.index, call.count = idx.ctypes.data, idx.size
    for name, value in fields.items():
        if isinstance(value, np.ndarray):
            keep.append(value)
            value = value.ctypes.data
        setattr(call, name, value)
    return call, keep


def _emu_call(entry, frames, delta, n_ac, **call):
    """One gray call through the host library: fills an EmuCall (_fill_call), runs `entry` (emu_embed_call, emu_extract_call or
    emu_readback_call) and -> the EmuResult"""
    lib = hostemu()
    call, keep = _fill_call(frames.shape, delta, n_ac, **call)
    res = EmuResult(size=ctypes.sizeof(EmuResult))
    if getattr(lib, entry)(ctypes.byref(call), ctypes.byref(res)) != 0:
        raise RuntimeError("EmuCall / EmuResult differ from tests/hostemu/emu_call.h: rebuild tests/hostemu or mend the mirror")
    assert res.used != 2 ** 64 - 1, "the host library refused the selection"
    return res


def _frames3(frames, copy=False):
    frames = frames if frames.ndim == 3 else frames[None]
    return np.array(frames, np.uint8, order="C") if copy else np.ascontiguousarray(frames)


def _block_map(frames):
    f, h, w = frames.shape
    return np.zeros(f * (h // 8) * (w // 8), np.uint8)


def host_embed_call(frames, delta, n_ac, bits, **call):
    """a gray embed call on the host -> (stego, EmuResult, replay map: bool per block in raster order over the batch - the
    guard handed the block to the exact replay).  call: see _emu_call."""
    frames = _frames3(frames)
    out, rmap = np.empty_like(frames), _block_map(frames)
    res = _emu_call("emu_embed_call", frames, delta, n_ac, bits=bits, frames_in=frames, frames_out=out, replay_map=rmap, **call)
    return out, res, rmap.astype(bool)


def host_extract_call(frames, delta, n_ac, **call):
    """a gray extract call on the host -> (0/1 per bit, EmuResult, candidate map: bool per block - with extract_wave set, step
    one of FAST extraction flags the block)"""
    frames = _frames3(frames)
    index = call.get("index")
    n = max(0, min(int(n_ac), 63)) if index is None else len(index)
    cmap = _block_map(frames)
    out = np.zeros(cmap.size * max(n, 1), np.uint8)
    res = _emu_call("emu_extract_call", frames, delta, n_ac, frames_in=frames, bits_out=out, candidate_map=cmap, **call)
    return out[:res.used], res, cmap.astype(bool)


def host_soft_args(shape, delta, n_ac, **call):
    """the SoftArgs the launch of an extract call over frames of `shape` passes -> dict(on, vote, hist, period, base, head, size)"""
    call, keep = _fill_call(shape, delta, n_ac, **call)
    fields = np.zeros(7, np.uint64)
    assert hostemu().emu_soft_args(ctypes.byref(call), fields.ctypes.data) == 0, "the host library refused the call"
    return dict(zip(("on", "vote", "hist", "period", "base", "head", "size"), map(int, fields)))


def host_readback_call(stego, delta, n_ac, bits, **call):
    """the read-back pass on the host over a copy of `stego` (one frame or a batch) -> (stego after the pass, (repaired,
    unrepaired), status per physical block: 0 reads back, 1 repaired, 2 left, 3 carries no payload)"""
    frames = _frames3(stego, copy=True)
    status = _block_map(frames)
    res = _emu_call("emu_readback_call", frames, delta, n_ac, bits=bits, guarded=True, frames_out=frames, status=status, **call)
    return (frames if stego.ndim == 3 else frames[0]), (int(res.repaired), int(res.unrepaired)), status


_SCALES = {"guard_scale": 1.0, "tie_scale": 1.0}


class emu_scales:
    """`with emu_scales(guard=s, tie=t):` - BETA / the tie margin of emu_embed / emu_extract (and the two maps) multiplied by
    s / t inside the block, as the experiments library's SVS_GUARD_SCALE / SVS_TIE_SCALE do (1 = the product's bounds)"""

    def __init__(self, guard=1.0, tie=1.0):
        self.guard, self.tie = float(guard), float(tie)

    def __enter__(self):
        _SCALES.update(guard_scale=self.guard, tie_scale=self.tie)
        return self

    def __exit__(self, *exc):
        _SCALES.update(guard_scale=1.0, tie_scale=1.0)
        return False


def emu_embed(frames, delta, n_ac, bits, bit_offset=0, exact=False, replayed=None):
    """`replayed`: optional list; receives the number of blocks FAST mode handed to the exact replay."""
    out, res, _ = host_embed_call(frames, delta, n_ac, bits, bit_offset=bit_offset, exact=int(exact), **_SCALES)
    if replayed is not None:
        replayed.append(int(res.replayed))
    return out, int(res.used)


def emu_replay_map(frames, delta, n_ac, bits):
    """-> bool per block (raster order over the batch): hostemu's guarded embed handed the block to the exact replay"""
    return host_embed_call(frames, delta, n_ac, bits, exact=0, **_SCALES)[2]


def emu_extract(frames, delta, n_ac, exact=False, redone=None, wave=0):
    """`redone`: optional list; receives the number of blocks FAST mode recomputed with the exact transform.  `wave` = 64:
    FAST extraction's step two for every block of a wave with a candidate, as the kernels do it (0: per block)."""
    out, res, _ = host_extract_call(frames, delta, n_ac, pocketfft=bool(exact), extract_wave=int(wave), **_SCALES)
    if redone is not None:
        redone.append(int(res.replayed))
    return out


def emu_tie_candidates(frames, delta, n_ac):
    """-> bool per block: step one of FAST extraction (n >= 8) flags the block as a candidate (wave mode of emu_extract)"""
    return host_extract_call(frames, delta, n_ac, extract_wave=64, **_SCALES)[2]


def guard_corpus_case(arrays, meta, name):
    """One setting of tests/golden/guard_corpus.npz (tests/golden/make_guard_corpus.py) as its frame is laid out:
    -> dict(frame uint8 [H, W], bits 0/1 [blocks * n] (embed settings only), positions, stars).  The file holds the corpus
    blocks, their payload bits and positions, a small filler library and each block's filler index; the frame is
    rebuilt from them (filler blocks carry all-zero payload bits)."""
    m = meta["embed"].get(name) or meta["extract"][name]
    h, w = meta["frame_shape"][0], m.get("width", meta["frame_shape"][1])
    blocks = arrays[name + "/filler"][arrays[name + "/filler_index"]]
    positions = arrays[name + "/positions"].astype(np.int64)
    corpus = arrays[name + "/blocks"]
    blocks[positions] = corpus
    frame = np.ascontiguousarray(blocks.reshape(h // 8, w // 8, 8, 8).transpose(0, 2, 1, 3).reshape(h, w))
    case = dict(frame=frame, positions=positions, stars=arrays[name + "/stars"])
    if name in meta["embed"]:
        n = m["n_ac"]
        bits = np.zeros((blocks.shape[0], n), np.uint8)
        bits[positions] = np.unpackbits(arrays[name + "/bits"], count=len(positions) * n).reshape(-1, n)
        case["bits"] = bits.reshape(-1)
    return case


def guarded_soak_cases(count=64, seed=77):
    """Random (frames, delta, n_ac, bits, bit_offset, n_bits) cases for the GUARDED mode: shapes with odd and even block
    counts per row, partial waves, budgets ending inside a block, bit offsets, every n <= 15 (every eighth case above, where
    the exact kernels run), quantiser steps of all three evaluation kinds (power of two, float32, not a float32) across the
    guard's delta range and outside it, frames mixing noise with flat, dark, saturated and smooth areas."""
    rng = np.random.default_rng(seed)
    steps = [8, 0.5, 2, 20, 7.5, 13, 0.3, 0.7, 1.1, 100, 1000.5, 4096, 0.25, 0.2, 5000, 3.3]
    for it in range(count):
        f = int(rng.integers(1, 5))
        h, w = 8 * int(rng.integers(1, 14)), 8 * int(rng.integers(1, 36))
        n_ac = int(rng.integers(1, 16)) if it % 8 else int(rng.integers(16, 64))
        delta = steps[it % len(steps)]
        frames = rng.integers(0, 256, (f, h, w), dtype=np.uint8)
        kind = it % 5
        if kind == 1:
            frames[:, : h // 2] = int(rng.integers(0, 256))                 # flat area
        elif kind == 2:
            frames //= 32                                                    # dark: clipping at 0
        elif kind == 3:
            frames[:] = 255 - frames // 32                                   # bright: clipping at 255
        elif kind == 4:
            yy, xx = np.mgrid[0:h, 0:w]
            frames[:] = np.clip(40 + 0.8 * xx + 0.5 * yy + frames // 64, 0, 255).astype(np.uint8)
        cap = f * (h // 8) * (w // 8) * min(n_ac, 63)
        off = int(rng.integers(0, 70))
        n_bits = cap if it % 3 == 0 else int(rng.integers(0, cap + 9))
        bits = rng.integers(0, 2, off + n_bits).astype(np.uint8)
        yield it, frames, delta, n_ac, bits, off, n_bits, cap
