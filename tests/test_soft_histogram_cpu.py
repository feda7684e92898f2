"""The fused per-frame soft histograms without a GPU (include/svsdct.h, svs_soft_histogram*): the declarations, the refusals of
the two entry points through the real library (none reaches the device), the NumPy model of the format (svsdct/soft.py:
byte_histogram, margins, lattice_share) against numpy.bincount and soft.margin_histogram, the host build of the histogram's
integer side (tests/hostemu: the plan and the split of a wave's run of blocks into per-frame runs) against Python
integers, a whole call's counts through the host walker against the model's, and the scenario of examples/find_payload_frames.py on the model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dither_lib as dl
import soft_histogram_lib as hl
import soft_lib as sl
from svsdct import native
from svsdct import soft as sv
from testlib import REPO, hostemu

SYMBOLS = ("svs_soft_histogram_dev", "svs_soft_histogram")


# ---- declarations ----------------------------------------------------------------------------------------------------------
def test_both_calls_are_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "svsdct.h")).read()
    lib = native.load()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in native.SIGNATURES
        assert getattr(lib, name).argtypes == native.SIGNATURES[name][1]
    assert len(native.SIGNATURES[SYMBOLS[0]][1]) == len(native.SIGNATURES[SYMBOLS[1]][1]) + 1      # the stream
    assert re.search(r"#define\s+SVS_ABI_VERSION\s+4\b", header)
    assert lib.svs_abi_version() == native.ABI_VERSION == 4


def test_the_header_says_why_there_is_no_order_argument():
    header = open(os.path.join(REPO, "include", "svsdct.h")).read()
    section = header[header.index("fused per-frame soft histograms"): header.index("int svs_soft_histogram_dev")]
    assert "svs_block_order" in section and "a frame embedded" in section and "under an order is read with this same call" in section
    for name in SYMBOLS:
        decl = header[header.index("int %s(" % name):]
        assert "svs_block_order" not in decl[: decl.index(";")]
    from svsdct import batch
    for fn in (batch.extract_histogram_frames, batch.extract_histogram_device):
        assert "block_key" not in fn.__code__.co_varnames[: fn.__code__.co_argcount] and "order" in fn.__doc__


# ---- refusals through the real library: none reaches the device ------------------------------------------------------------
FAKE_IN, FAKE_HIST = 0x10000, 0x20000       # never dereferenced: every case returns before any device work
SENTINEL = 0xA5A5A5A5
SMALL = (1, 16, 16, 0, 16, 256)
# 8 260 x 8 260 = 68 227 600 blocks pass the geometry checks (below 2^31); times 63 they exceed 2^32 - 1
WIDE = (1, 66080, 66080, 0, 66080, 66080 * 66080)


def _coeffs(count, index):
    return native.Coeffs(count, (C.c_uint8 * 63)(*index))


def _call(lib, dev, planes=SMALL, gray=FAKE_IN, hist="own", coeffs=None, dither=None, delta=8.0, n_ac=10, flags=0):
    """-> (rc, message, *n_bits_out, the host rows after the call or None).  hist: "own" - the device form gets a fake device
    pointer, the host form a real array of sentinels for the planes' frames; None; or an address."""
    pl = native.Planes(*planes)
    d = native.Dither(*dither) if dither else None
    host = None
    if hist == "own":
        if dev:
            hist = FAKE_HIST
        else:
            host = np.full(256 * max(1, planes[0]), SENTINEL, np.uint32)
            hist = host.ctypes.data
    got = C.c_uint64(0xDEAD)
    ref = lambda s: C.byref(s) if s is not None else None    # noqa: E731
    args = [gray, C.byref(pl), ref(coeffs), ref(d), float(delta), int(n_ac), hist, flags, C.byref(got)]
    rc = getattr(lib, SYMBOLS[0] if dev else SYMBOLS[1])(*args, *([None] if dev else []))
    return rc, "" if rc == 0 else lib.svs_last_error().decode(), int(got.value), host


REFUSALS = [
    ("SVS_NEAREST", dict(flags=native.SVS_NEAREST), "flags"),
    ("SVS_MINMOVE", dict(flags=native.SVS_MINMOVE), "flags"),
    ("SVS_READBACK", dict(flags=native.SVS_READBACK), "flags"),
    ("unknown flag", dict(flags=0x400), "flags"),
    ("delta 0", dict(delta=0.0), "delta"),
    ("delta -1", dict(delta=-1.0), "delta"),
    ("coeffs.count", dict(coeffs=_coeffs(64, [1])), "svs_coeffs.count"),
    ("coeffs behind count", dict(coeffs=_coeffs(2, [1, 2, 3])), "svs_coeffs.index"),
    ("coeffs twice", dict(coeffs=_coeffs(2, [5, 5])), "svs_coeffs.index"),
    ("coeffs DC", dict(coeffs=_coeffs(2, [0, 5])), "svs_coeffs.index"),
    ("dither.reserved", dict(dither=(1, 0, 1)), "svs_dither.reserved"),
    ("planes.reserved", dict(planes=(1, 16, 16, 1, 16, 256)), "svs_planes.reserved"),
    ("planes height", dict(planes=(1, 12, 16, 0, 16, 192)), "multiples of 8"),
    ("planes row_pitch", dict(planes=(1, 16, 16, 0, 8, 256)), "row_pitch"),
    ("planes frame_pitch", dict(planes=(2, 16, 16, 0, 16, 128)), "frame_pitch"),
    ("planes frames", dict(planes=(-1, 16, 16, 0, 16, 256)), "geometry"),
    ("gray NULL", dict(gray=None), "pointer is NULL"),
    ("hist NULL", dict(hist=None), "pointer is NULL"),
    ("a frame above 2^32 - 1 bytes", dict(planes=WIDE, n_ac=63), "2^32 - 1"),
]


@pytest.mark.parametrize("dev", (True, False), ids=("dev", "host"))
@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals_come_before_any_device_work_and_leave_the_out_parameters(case, dev):
    _, kw, text = case
    rc, message, got, host = _call(native.load(), dev, **kw)
    assert rc == native.SVS_ERR_INVALID_ARG and text in message, (rc, message)
    assert got == 0xDEAD                                     # *n_bits_out: untouched
    assert host is None or (host == SENTINEL).all()          # the host form's rows: untouched


def test_an_unaligned_device_hist_is_refused():
    lib = native.load()
    for off in (1, 2, 3):
        rc, message, got, _ = _call(lib, True, hist=FAKE_HIST + off)
        assert rc == native.SVS_ERR_INVALID_ARG and "hist pointer must be 4-byte aligned" in message and got == 0xDEAD
    assert _call(lib, True, gray=FAKE_IN + 4)[0] == native.SVS_ERR_INVALID_ARG


def test_the_count_bound_is_on_the_bytes_of_one_frame():
    """68 227 600 blocks a frame: 62 coefficients stay below 2^32, 63 do not - and the planes pass the geometry checks, which
    refuse from 2^31 blocks on.  The accepted side cannot be called without a device; only the refused side is pinned."""
    blocks = (66080 // 8) ** 2
    assert blocks == 68_227_600 < 1 << 31 and blocks * 62 < 1 << 32 <= blocks * 63
    rc, message, got, _ = _call(native.load(), True, planes=WIDE, coeffs=_coeffs(63, range(1, 64)))
    assert rc == native.SVS_ERR_INVALID_ARG and "2^32 - 1" in message and got == 0xDEAD


@pytest.mark.parametrize("dev", (True, False), ids=("dev", "host"))
def test_the_empty_call_is_ok(dev):
    lib = native.load()
    for kw in (dict(planes=(0, 16, 16, 0, 16, 256)), dict(n_ac=0), dict(n_ac=-3), dict(planes=(0, 16, 16, 0, 16, 256), gray=None),
               dict(planes=(3, 16, 16, 0, 16, 256), n_ac=0, flags=native.SVS_EXACT_POCKETFFT | native.SVS_EXACT_GUARDED)):
        rc, message, got, host = _call(lib, dev, **kw)
        assert (rc, message, got) == (native.SVS_OK, "", 0), kw
        if host is not None:                                  # the host form writes its n_frames * 256 values: all zero
            n = 256 * kw.get("planes", SMALL)[0]
            assert not host[:n].any() and (host[n:] == SENTINEL).all(), kw
    assert _call(lib, dev, n_ac=0, hist=None)[:3] == (native.SVS_OK, "", 0)


def test_python_level_raises_before_the_library_is_loaded():
    from svsdct import batch
    frames = np.zeros((1, 16, 16), np.uint8)
    with pytest.raises(ValueError):
        batch.extract_histogram_frames(frames, 8, 10, coeffs=[1, 2, 3])           # len != n_ac
    for fn, args in ((batch.extract_histogram_frames, (frames, 8, 10)),
                     (batch.extract_histogram_device, (0, native.Planes.contiguous(1, 16, 16), 8, 10, 0))):
        with pytest.raises(TypeError):
            fn(*args, block_key=5)


# ---- the model of the format ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames,per", ((1, 1), (1, 640), (3, 7), (5, 1200), (70, 10)))
def test_byte_histogram_is_bincount_per_frame(frames, per):
    a = np.random.default_rng(frames * per).integers(0, 256, frames * per).astype(np.uint8)
    h = sv.byte_histogram(a, frames)
    assert h.dtype == np.int64 and h.shape == (frames, 256) and (h.sum(1) == per).all()
    for f in range(frames):
        assert np.array_equal(h[f], np.bincount(a[f * per: (f + 1) * per], minlength=256)), f
    assert np.array_equal(h[:, 128:].sum(1), (a >> 7).reshape(frames, per).sum(1))          # the hard ones
    assert np.array_equal(sv.margins(h), sv.margin_histogram(a, frames))
    assert sv.margins(h.astype(np.uint32)).dtype == np.int64
    share = sv.lattice_share(h)
    assert share.dtype == np.float64 and np.allclose(share, ((a & 127) >= 64).reshape(frames, per).mean(1), rtol=0, atol=1e-15)
    assert np.array_equal(sv.lattice_share(h, 0), np.ones(frames)) and not sv.lattice_share(h, 128).any()


def test_the_model_refuses_what_is_not_whole_frames_or_no_histogram():
    with pytest.raises(ValueError):
        sv.byte_histogram(np.zeros(7, np.uint8), 2)
    with pytest.raises(ValueError):
        sv.byte_histogram(np.zeros(4, np.uint8), 0)
    with pytest.raises(TypeError):
        sv.byte_histogram(np.zeros(4, np.int32), 2)
    with pytest.raises(TypeError):
        sv.margins(np.zeros((2, 128), np.int64))
    with pytest.raises(TypeError):
        sv.lattice_share(np.zeros((2, 256), np.float64))
    with pytest.raises(ValueError):
        sv.lattice_share(np.zeros((2, 256), np.int64), 129)
    h = sv.byte_histogram(np.array([0x85, 5, 127, 0x80], np.uint8), 2)
    assert h[0, 0x85] == 1 and h[0, 5] == 1 and h[1, 127] == 1 and h[1, 128] == 1 and h.sum() == 4
    assert np.isnan(sv.lattice_share(np.zeros((1, 256), np.uint32))[0])


def test_lattice_share_of_the_models_stego_and_cover():
    """the frames and seeds of tests/test_soft_extract_cpu.py (stego_set, test_comb_share): 1.000 for lattice stego and for
    dithered stego read with its key; a fair coin - 0.5 +- 0.05 is ten standard deviations at 2 400 samples - for dithered stego
    read without the key and for the never-embedded cover"""
    from oracle.qim_dct_oracle import frame_embed
    key = 0x5EED0FD17E12
    cover = dl.noise((96, 160), 64, 192, seed=21)
    pay = dl.payload(2400, seed=4)
    _, stego, used = frame_embed(cover, 20, pay, 10)
    dithered, used_d = dl.model_embed(cover, 20, pay, 10, key=key)
    assert used == used_d == 2400
    plain = np.concatenate([sl.model_soft(f, 20, 10) for f in (stego, dithered, cover)])
    keyed = np.concatenate([sl.model_soft(f, 20, 10, key=key) for f in (stego, dithered, cover)])
    s_plain, s_keyed = sv.lattice_share(sv.byte_histogram(plain, 3)), sv.lattice_share(sv.byte_histogram(keyed, 3))
    print("share of m >= 64 without a key: stego %.3f, dithered stego %.3f, cover %.3f; with the key: %.3f, %.3f, %.3f"
          % (*s_plain, *s_keyed))
    assert s_plain[0] == 1.0 and s_keyed[1] == 1.0
    for share in (s_plain[1], s_plain[2], s_keyed[0], s_keyed[2]):
        assert 0.45 <= share <= 0.55


# ---- the integer side of the kernel's histogram tail on the host (tests/hostemu) --------------------------------------------
def test_a_histogram_call_plans_the_soft_side_with_the_histogram_on_and_never_keyed():
    for delta in (8, 20, 12.5, 0.1):
        for n in (1, 10, 63):
            for keyed in (False, True):
                plan, args, size = hl.host_hist_args(delta, n, keyed)
                assert plan == dict(path=sl.PATH_EXACT, rows=8, soft=1, vote=0, hist=1, keyed=0)
                assert args == dict(on=1, vote=0, hist=1)
    assert size == 56                                        # SoftArgs keeps the vote's size: the field took the pad word
    assert hostemu().emu_hist_bins() == 256
    # a soft call and a vote call leave the field off
    import soft_vote_lib as vl
    assert vl.host_vote_args(20, 10, 2400, 0)[0]["vote"] == 1 and sl.host_plan(20, 10)["soft"] == 1


@pytest.mark.parametrize("bpf", (1, 2, 6, 63, 64, 65, 120, 255, 256, 257))
def test_the_per_frame_runs_of_every_wave_are_pythons(bpf):
    """every wave start of the first three workgroups, a total that ends on a frame and totals with a ragged last wave and a
    ragged last workgroup: the runs the tail walks (frame_run over the workgroup's frames) against Python integers, and what
    they must add up to - every live block of the wave once, in the frame Python's division puts it in"""
    totals = {3 * hl.WG, 3 * hl.WG - 1, 2 * hl.WG + 65, 2 * hl.WG + 1, 64 * 7 + 13, -(-(2 * hl.WG + 30) // bpf) * bpf, bpf, 1}
    for total in sorted(t for t in totals if t >= 1):
        for wg_first in range(0, 3 * hl.WG, hl.WG):
            for wave_first in range(wg_first, wg_first + hl.WG, 64):
                got = hl.host_runs(wg_first, wave_first, total, bpf)
                assert got == hl.python_runs(wg_first, wave_first, total, bpf), (bpf, total, wave_first)
                if wg_first >= total:
                    assert got == []
                    continue
                live = range(wave_first, max(wave_first, min(wave_first + 64, total)))
                covered = [(f, wave_first + t) for f, b, e in got for t in range(b, e)]
                assert covered == [(g // bpf, g) for g in live], (bpf, total, wave_first)
                assert all(0 <= b <= e <= 64 for _, b, e in got)
                frames = [f for f, _, _ in got]               # the same frames for the four waves: the barriers line up
                assert frames == list(range(wg_first // bpf, (min(wg_first + hl.WG, total) - 1) // bpf + 1))


def test_frame_run_far_into_a_large_call():
    """blocks near 2^31 (the most a call holds) at 4K's 129 600 blocks per frame: no 32-bit product wraps"""
    bpf = 129600
    total = (1 << 31) - 1
    for wg_first in (total - total % hl.WG, (16570 * bpf) // hl.WG * hl.WG):
        for wave_first in range(wg_first, wg_first + hl.WG, 64):
            assert hl.host_runs(wg_first, wave_first, total, bpf) == hl.python_runs(wg_first, wave_first, total, bpf)


@pytest.mark.parametrize("form", ("prefix", "dither+zigzag"))
@pytest.mark.parametrize("name", [k for k, (f, h, w) in hl.SHAPES.items() if (h // 8) * (w // 8) <= 257])
def test_the_walkers_histogram_is_the_models(name, form):
    """a whole histogram call through the product headers on the host - extract_block_soft with the launch's tables, every byte
    counted into its frame's row - against soft.byte_histogram of the NumPy model's bytes, exactly"""
    delta, n, key, first_frame = 20, 10, 0x5EED0FD17E12, 3
    frames = dl.noise(hl.SHAPES[name], 0, 256, seed=9)
    keyed = form != "prefix"
    kw = dict(index=sl.zigzag(n), key=key, first_frame=first_frame) if keyed else {}
    call = dict(index=sl.zigzag(n), dither_key=key, first_frame=first_frame) if keyed else {}
    got = hl.host_hist(frames, delta, n, **call)
    want = sv.byte_histogram(sl.model_batch_soft(frames, delta, n, **kw), frames.shape[0])
    assert got.dtype == np.uint32 and np.array_equal(got, want), (name, form)
    assert int(got.sum()) == frames.shape[0] * (frames.shape[1] // 8) * (frames.shape[2] // 8) * n


# ---- the use: which frames carry a payload (examples/find_payload_frames.py) on the model ----------------------------------
def test_the_scenario_stays_inside_its_bounds_on_the_model():
    """eight frames of 240 x 320 noise, a dithered full-capacity payload in frames 2..4 only (the dither's first_frame is the
    clip's frame index): with the key the share of m >= 64 is 1.0 there and a fair coin elsewhere, without it a fair coin
    everywhere - 0.5 +- 0.05 is eleven standard deviations at 12 000 bytes a frame.  The seed is fixed: the GPU tier asserts the
    same bounds on the same frames."""
    s = hl.SCENARIO
    clip = hl.scenario_stego_model()
    keyed = sl.model_batch_soft(clip, s["delta"], s["n_ac"], key=s["key"])
    keyless = sl.model_batch_soft(clip, s["delta"], s["n_ac"])
    with_key, without = sv.lattice_share(sv.byte_histogram(keyed, s["frames"])), sv.lattice_share(sv.byte_histogram(keyless, s["frames"]))
    print("lattice share with the key:", np.round(with_key, 3).tolist(), "without:", np.round(without, 3).tolist())
    hl.assert_scenario(with_key, without)
