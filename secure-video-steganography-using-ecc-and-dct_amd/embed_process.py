"""Drop-in module: `embed_gambar_ke_video_final` with the reference's signature and return values
(reference embed_process.py:17-152), its frame loop (:108-144) run as batched GPU launches.

Host work kept on the host (north-star): secret image -> bits (helpers), SHA3 / ECDH / HKDF /
AES-GCM (config_and_setup), OpenCV decode + FFV1 encode.  GPU work: every frame that carries payload
goes through `svsdct.batch.embed_frames` in batches of SVS_BATCH_FRAMES frames - frame k of the clip
takes stream bits [k*cap, (k+1)*cap), exactly what the reference's per-frame calls hand out
(:116-128), so the stego frames are the ones a frame-by-frame loop would produce.
"""
from __future__ import annotations

import os

import numpy as np

import helpers as steg_helpers
from config_and_setup import (bitstream_ke_bytes, buat_pasangan_kunci_ecc, buat_shared_secret_ecdh,
                              derive_kunci_aes_dari_shared_secret, deserialisasi_kunci_publik_ecc_compressed,
                              enkripsi_aes_gcm, hitung_sha3_256, persiapkan_file_input,  # noqa: F401
                              serialisasi_kunci_publik_ecc_compressed, setup_kunci_ecc)  # noqa: F401
from svsdct import batch as _batch
from svsdct import coeffs as _coeffs
from svsdct import dither as _dither
from svsdct import framing as _framing
from svsdct import order as _order
from svsdct import matrix as _matrix
from svsdct import steps as _steps
from svsdct.pipeline import FramePipeline, SlotFeeder, read_ahead

BATCH_FRAMES = int(os.environ.get("SVS_BATCH_FRAMES", "32"))
PIPELINE_DEPTH = int(os.environ.get("SVS_PIPELINE_DEPTH", "3"))     # batches in flight between decode and encode
# SVS_FUSED_COLOUR=1: colour frames go to the GPU as they are and BGR -> gray -> embed -> BGR runs as ONE kernel
# (svs_embed_bgr_dev) instead of cv2.cvtColor on the host either side of the operator (:117-126).  Only used when the
# device conversion reproduces this machine's cv2 bit for bit (svsdct.colour); otherwise the host conversion stays.
FUSED_COLOUR = os.environ.get("SVS_FUSED_COLOUR", "0") == "1"
# SVS_KEEP_COLOUR=1 (implies SVS_FUSED_COLOUR, behind the same cv2 check): the frames that carry payload keep the cover's
# colours - each pixel shifted to the stego gray (SVS_KEEP_COLOUR, include/svsdct.h) - instead of the reference's
# COLOR_GRAY2BGR.  Their BGR2GRAY is the reference's stego plane, so the receiver extracts the same bits.
KEEP_COLOUR = os.environ.get("SVS_KEEP_COLOUR", "0") == "1"
# SVS_BLOCK_KEY=<integer, int(x, 0)> (read per call): keyed block order - the blocks of video frame k take that frame's bits
# in a key-seeded order (svsdct/order.py, include/svsdct.h) instead of raster order from the top-left block, so a payload
# that fills part of a frame is spread over all of it.  The receiver needs the same key.  Unset: the reference's order, byte
# for byte.  Not with SVS_KEEP_COLOUR (the fused colour kernels have no keyed form: refused); with SVS_FUSED_COLOUR the
# host-conversion gray path runs.
# SVS_READBACK=1 (opt-in): every frame block that carries payload is read back with the reference's extraction, and a block
# that the reference's clipping or truncation made unreadable (letterbox bars, flat black or white areas) is repaired
# (SVS_READBACK, include/svsdct.h) - otherwise one such block makes the receiver's AES-GCM reject the payload.  Repaired blocks
# are no longer the reference's pixels.  One line reports the totals, and a warning names blocks left unrepaired.  The gray
# path only: refused together with SVS_FUSED_COLOUR / SVS_KEEP_COLOUR (the colour form has a switch of its own, below).
READBACK = os.environ.get("SVS_READBACK", "0") == "1"
# SVS_READBACK_COLOUR=1 (opt-in): the same read-back and repair on the fused colour path (svs_embed_bgr_readback,
# include/svsdct.h).  Implies SVS_FUSED_COLOUR behind the same cv2 check and combines with SVS_KEEP_COLOUR: repaired blocks keep
# the cover's colours, shifted to the repaired gray.  Where the cv2 check fails the gray read-back path runs instead (its
# output is the plain colour form's, byte for byte).  Refused together with SVS_BLOCK_KEY (no keyed colour form) and with
# SVS_READBACK (one switch per path).
READBACK_COLOUR = os.environ.get("SVS_READBACK_COLOUR", "0") == "1"
# SVS_READBACK_KEYED=1 (opt-in): the read-back and repair under SVS_COEFFS and / or SVS_DITHER_KEY (svs_embed_dithered_readback,
# include/svsdct.h): every payload block is read back as the receiver's selected / dithered extraction will read it, and
# repaired where clipping or truncation lost a bit.  The gray path, with SVS_BLOCK_KEY, SVS_NEAREST and SVS_MINMOVE; with
# neither a selection nor a dither it is SVS_READBACK's pass.  Refused together with SVS_READBACK and SVS_READBACK_COLOUR (one
# switch per path) and with SVS_KEEP_COLOUR; with SVS_FUSED_COLOUR the host-conversion gray path runs.  The same one-line report.
READBACK_KEYED = os.environ.get("SVS_READBACK_KEYED", "0") == "1"
# SVS_READBACK_STEPPED=1 (opt-in): the read-back and repair under SVS_STEPS (svs_stepped_embed_readback, include/svsdct.h): every
# payload block is read back as the receiver's stepped extraction will read it, and repaired where clipping or truncation lost
# a bit.  It needs SVS_STEPS (refused without it) and is the gray path's, with SVS_BLOCK_KEY, SVS_COEFFS, SVS_DITHER_KEY,
# SVS_NEAREST and SVS_MINMOVE.  Refused together with SVS_READBACK, SVS_READBACK_COLOUR and SVS_READBACK_KEYED (one switch per
# path) and with SVS_KEEP_COLOUR; with SVS_FUSED_COLOUR the host-conversion gray path runs.  The same one-line report.
READBACK_STEPPED = os.environ.get("SVS_READBACK_STEPPED", "0") == "1"
# SVS_READBACK_MARGIN=g (opt-in, an integer 1..127): SVS_READBACK_STEPPED's pass followed by the soft-margin pass
# (svs_stepped_embed_readback_margin, include/svsdct.h): a block that decodes but would reach the receiver with a soft margin
# m < g on some payload coefficient is searched for bytes that are strong throughout.  It implies SVS_READBACK_STEPPED=1 and, as
# that switch, needs SVS_STEPS.  The report line gains the two counts of the pass: blocks strengthened, blocks left weak.
READBACK_MARGIN = os.environ.get("SVS_READBACK_MARGIN", "")
# SVS_NEAREST=1 (opt-in): a coefficient whose parity has to change moves to the nearer of its two neighbouring lattice points
# instead of the reference's fixed direction (SVS_NEAREST, include/svsdct.h): about 2 dB more PSNR at the same delta.  The stego
# frames are no longer the reference's pixels; the receiver does not change.  Allowed with every other switch.
NEAREST = os.environ.get("SVS_NEAREST", "0") == "1"
# SVS_MINMOVE=1 (opt-in): a payload coefficient moves only as far as the decision cell of its index asks, less a margin that
# covers the truncation of the stego pixels, and stays put when it is already there (SVS_MINMOVE, include/svsdct.h): 4 to 7 dB
# more PSNR at delta >= 12 (CPU-measured).  The stego frames are neither the reference's nor SVS_NEAREST's pixels; the receiver
# does not change.  Implies the nearest direction.  Blocks that clip at 0 / 255 are outside its guarantee: SVS_READBACK=1 is the
# remedy and combines with it.  Allowed with every other switch.
MINMOVE = os.environ.get("SVS_MINMOVE", "0") == "1"
# SVS_COEFFS (read per call, opt-in): which coefficients of a block carry the payload (svsdct/coeffs.py) - "zigzag",
# "zigzag:<first scan position>", "rowmajor" or a comma-separated list of num_ac_coeffs distinct flat indices in 1..63.  Unset:
# the reference's row-major coefficients 1..num_ac_coeffs, today's bytes.  The receiver must set the same value.  The gray path
# only (with SVS_FUSED_COLOUR the host-conversion gray path runs); refused together with SVS_KEEP_COLOUR, SVS_READBACK and
# SVS_READBACK_COLOUR (a selection has no colour form; its read-back is SVS_READBACK_KEYED=1).  Allowed with SVS_BLOCK_KEY and
# SVS_NEAREST.
# SVS_DITHER_KEY=<integer, int(x, 0)> (read per call, opt-in): keyed dither modulation (svsdct/dither.py, include/svsdct.h) - the
# quantiser lattice of every payload coefficient of video frame k is shifted by an offset derived from the key, k, the block and
# the coefficient: no comb in the coefficient histogram, no bits for a receiver without the key, no distortion cost.  Unset:
# no dither, today's bytes and routes.  The receiver must set the same value.  The gray path only (with SVS_FUSED_COLOUR the
# host-conversion gray path runs); refused together with SVS_KEEP_COLOUR, SVS_READBACK and SVS_READBACK_COLOUR (a dithered call
# has no colour form; its read-back is SVS_READBACK_KEYED=1).  Allowed with SVS_BLOCK_KEY, SVS_COEFFS, SVS_NEAREST and
# SVS_MINMOVE.
# SVS_STEPS (read per call, opt-in): per-coefficient QIM steps (svsdct/steps.py, include/svsdct.h) - `q<quality>x<multiple>`,
# optionally `f<floor>` (q75x2, q95x2f16: the steps of an 8x8 intra codec at that quality times the multiple, none below the
# floor), or 64 comma-separated integers.  Coefficient k is quantised with its own step and DELTA is not used; a lattice point of
# a matched table passes that codec's requantiser unchanged.  Unset: today's bytes and routes.  The receiver must set the same
# value.  The gray path only (with SVS_FUSED_COLOUR the host-conversion gray path runs); refused together with SVS_KEEP_COLOUR,
# SVS_READBACK, SVS_READBACK_COLOUR and SVS_READBACK_KEYED (a stepped call has no colour form; its read-back is
# SVS_READBACK_STEPPED=1).  Allowed with
# SVS_BLOCK_KEY, SVS_COEFFS, SVS_DITHER_KEY, SVS_NEAREST and SVS_MINMOVE.
# SVS_MATRIX (read per call, opt-in): matrix embedding (svsdct/matrix.py, include/svsdct.h) - `k` (1..6) or `k:pair` (k <= 5).  A
# block carries k bits as the Hamming syndrome of the parities of its 2^k - 1 payload coefficients (the AC count or SVS_COEFFS
# must name exactly that many), so at most one of them - with `:pair` the cheaper of one or two - changes parity; the capacity of
# a frame becomes blocks * k.  It needs SVS_STEPS (refused without it; `20,20,..` 64 times for one delta) and pays off with
# SVS_MINMOVE=1.  Refused with every read-back switch.  The receiver must set the same k.


def _keyed(block_key=None, dither_key=None, **kw):
    """keyword arguments of a keyed call (block order, dither): none at all without a key, so the unkeyed loop makes exactly the
    calls it made before the order and the dither existed"""
    if block_key is None and dither_key is None:
        return {}
    return kw if kw else {"block_key": block_key}


def _cv2():
    import cv2
    return cv2


def _siapkan_payload(path_gambar_rahasia, kunci_publik_penerima_compressed):
    """Secret image -> framed, encrypted payload bits (reference :25-74).  Returns None after printing the
    reason when a stage fails, like the reference's early `return False, None, None` exits."""
    lebar, tinggi, bit_gambar = steg_helpers.gambar_ke_bitstream(path_gambar_rahasia)
    if bit_gambar is None:
        return None
    try:
        plaintext = bitstream_ke_bytes(bit_gambar)
    except ValueError as exc:
        print(f"  Error: Konversi bitstream gambar ke bytes gagal: {exc}")
        return None
    print("\n  [Tahap Embedding 1: Persiapan Kriptografi]")
    digest = hitung_sha3_256(plaintext)
    print(f"      Hash SHA3-256 ({len(digest)} bytes) dibuat.")
    try:
        eph_priv, eph_pub = buat_pasangan_kunci_ecc()
        penerima = deserialisasi_kunci_publik_ecc_compressed(kunci_publik_penerima_compressed)
        salt = os.urandom(16)
        kunci_aes = derive_kunci_aes_dari_shared_secret(buat_shared_secret_ecdh(eph_priv, penerima), salt, 32)
        eph_pub_bytes = serialisasi_kunci_publik_ecc_compressed(eph_pub)
        print("      Kunci AES berhasil diderivasi dari shared secret ECC.")
    except Exception as exc:
        print(f"    Error: Setup ECC atau derivasi kunci AES gagal: {exc}")
        return None
    try:
        ciphertext, nonce, tag = enkripsi_aes_gcm(plaintext, kunci_aes)
        print("      Gambar berhasil dienkripsi.")
    except Exception as exc:
        print(f"    Error: Enkripsi AES gagal: {exc}")
        return None
    print("\n  [Tahap Embedding 2: Membuat Payload Lengkap]")
    try:
        bits = _framing.build_payload_bits(lebar, tinggi, eph_pub_bytes, salt, digest, nonce, tag, ciphertext)
    except ValueError as exc:
        print(f"    Error: Gagal membuat payload: {exc}")
        return None
    print(f"    Total bit payload yang akan disisipkan: {bits.size} bits.")
    print(f"      - Metadata Gambar: {2 * _framing.DIM_BITS} bits (L:{lebar}, T:{tinggi})")
    print(f"      - Header kunci/salt/hash/nonce/tag: {_framing.HEADER_BITS_STANDARD - 2 * _framing.DIM_BITS - 32} bits")
    print(f"      - Info Ciphertext: {32 + 8 * len(ciphertext)} bits")
    return bits


def embed_gambar_ke_video_final(path_video_input, path_gambar_rahasia, path_video_output_base,
                                delta_kuantisasi, num_ac_coeffs,
                                kunci_publik_ecc_penerima_bytes_compressed):
    """Embed the (encrypted) secret image into the video.  -> (True, first_gray, first_stego) when the whole
    payload was embedded, else (False, None, None).  Output is always '<base>.avi', FFV1, colour frames."""
    print("\n=== MEMULAI PROSES EMBEDDING GAMBAR KE VIDEO ===")
    print(f"  Gambar Rahasia: '{path_gambar_rahasia}'")
    print(f"  Video Input: '{path_video_input}'")
    print(f"  Parameter: DELTA={delta_kuantisasi}, Koefisien AC per Blok={num_ac_coeffs}")
    try:
        kunci_blok = _order.key_from_env()
    except (TypeError, ValueError) as exc:
        print(f"    Error: SVS_BLOCK_KEY tidak valid ({exc}).")
        return False, None, None
    try:
        pilihan = _coeffs.from_env(_batch.clamp_ac(num_ac_coeffs))
    except (TypeError, ValueError) as exc:
        print(f"    Error: SVS_COEFFS tidak valid ({exc}).")
        return False, None, None
    try:
        kunci_dither = _dither.key_from_env()
    except (TypeError, ValueError) as exc:
        print(f"    Error: SVS_DITHER_KEY tidak valid ({exc}).")
        return False, None, None
    try:
        tabel_langkah = _steps.from_env()
    except (TypeError, ValueError) as exc:
        print(f"    Error: SVS_STEPS tidak valid ({exc}).")
        return False, None, None
    if tabel_langkah is not None and (KEEP_COLOUR or READBACK or READBACK_COLOUR or READBACK_KEYED):
        print("    Error: SVS_STEPS tidak dapat dipakai bersama SVS_KEEP_COLOUR, SVS_READBACK, SVS_READBACK_COLOUR atau "
              "SVS_READBACK_KEYED.")
        return False, None, None
    if READBACK_STEPPED and tabel_langkah is None:
        print("    Error: SVS_READBACK_STEPPED=1 memerlukan SVS_STEPS.")
        return False, None, None
    if READBACK_STEPPED and (KEEP_COLOUR or READBACK or READBACK_COLOUR or READBACK_KEYED):
        print("    Error: SVS_READBACK_STEPPED tidak dapat dipakai bersama SVS_KEEP_COLOUR, SVS_READBACK, SVS_READBACK_COLOUR atau "
              "SVS_READBACK_KEYED.")
        return False, None, None
    try:
        matriks = _matrix.from_env()
    except (TypeError, ValueError) as exc:
        print(f"    Error: SVS_MATRIX tidak valid ({exc}).")
        return False, None, None
    if matriks is not None and tabel_langkah is None:
        print("    Error: SVS_MATRIX memerlukan SVS_STEPS.")
        return False, None, None
    if matriks is not None and (READBACK_STEPPED or READBACK_MARGIN):
        print("    Error: SVS_MATRIX tidak dapat dipakai bersama SVS_READBACK_STEPPED atau SVS_READBACK_MARGIN.")
        return False, None, None
    gerbang = None
    if READBACK_MARGIN:
        if tabel_langkah is None:
            print("    Error: SVS_READBACK_MARGIN memerlukan SVS_STEPS.")
            return False, None, None
        if not (READBACK_MARGIN.isdigit() and 1 <= int(READBACK_MARGIN) <= 127):
            print(f"    Error: SVS_READBACK_MARGIN harus bilangan bulat 1..127 (bukan '{READBACK_MARGIN}').")
            return False, None, None
        gerbang = int(READBACK_MARGIN)
    if kunci_dither is not None and (KEEP_COLOUR or READBACK or READBACK_COLOUR):
        print("    Error: SVS_DITHER_KEY tidak dapat dipakai bersama SVS_KEEP_COLOUR, SVS_READBACK atau SVS_READBACK_COLOUR.")
        return False, None, None
    if pilihan is not None and (KEEP_COLOUR or READBACK or READBACK_COLOUR):
        print("    Error: SVS_COEFFS tidak dapat dipakai bersama SVS_KEEP_COLOUR, SVS_READBACK atau SVS_READBACK_COLOUR.")
        return False, None, None
    if kunci_blok is not None and KEEP_COLOUR:
        print("    Error: SVS_BLOCK_KEY tidak dapat dipakai bersama SVS_KEEP_COLOUR.")
        return False, None, None
    if READBACK_KEYED and (READBACK or READBACK_COLOUR):
        raise ValueError("SVS_READBACK_KEYED=1 cannot be combined with SVS_READBACK=1 / SVS_READBACK_COLOUR=1: one switch per path")
    if READBACK_KEYED and KEEP_COLOUR:
        raise ValueError("SVS_READBACK_KEYED=1 cannot be combined with SVS_KEEP_COLOUR: the keyed read-back is the gray path's")
    if READBACK_COLOUR and READBACK:
        raise ValueError("SVS_READBACK_COLOUR=1 cannot be combined with SVS_READBACK=1: one switch per path")
    if READBACK_COLOUR and kunci_blok is not None:
        raise ValueError("SVS_READBACK_COLOUR=1 cannot be combined with SVS_BLOCK_KEY: the fused colour path has no keyed form")
    if READBACK and (FUSED_COLOUR or KEEP_COLOUR):
        raise ValueError("SVS_READBACK=1 cannot be combined with SVS_FUSED_COLOUR / SVS_KEEP_COLOUR: "
                         "the read-back of the fused colour path is SVS_READBACK_COLOUR=1")

    payload = _siapkan_payload(path_gambar_rahasia, kunci_publik_ecc_penerima_bytes_compressed)
    if payload is None:
        return False, None, None
    total_bits = int(payload.size)

    print("\n  [Tahap Embedding 3: Menyisipkan Payload ke Frame Video]")
    cv2 = _cv2()
    cap = cv2.VideoCapture(path_video_input)
    if not cap.isOpened():
        print(f"    Error: Video input '{path_video_input}' tidak bisa dibuka.")
        return False, None, None
    w_in, h_in = int(cap.get(cv2.CAP_PROP_FRAME_WIDTH)), int(cap.get(cv2.CAP_PROP_FRAME_HEIGHT))
    fps = cap.get(cv2.CAP_PROP_FPS)
    out_w, out_h = (w_in // 8) * 8, (h_in // 8) * 8                  # crop to whole blocks (:94)
    if out_w == 0 or out_h == 0:
        print("    Error: Dimensi video terlalu kecil.")
        cap.release()
        return False, None, None
    path_out = steg_helpers.get_avi_path(path_video_output_base)
    writer = cv2.VideoWriter(path_out, cv2.VideoWriter_fourcc(*"FFV1"), fps, (out_w, out_h), isColor=True)
    if not writer.isOpened():
        print(f"    ERROR: Gagal VideoWriter FFV1 '{path_out}'.")
        cap.release()
        return False, None, None
    print(f"    Video output akan disimpan sebagai '{path_out}' (Codec: FFV1).")

    tabel_warna = None
    if (FUSED_COLOUR or KEEP_COLOUR or READBACK_COLOUR) and kunci_blok is None and pilihan is None and kunci_dither is None \
            and not READBACK_KEYED and tabel_langkah is None:   # keyed order, selection, dither, keyed read-back, steps: the host-conversion gray path
        from svsdct import colour as _colour
        try:
            tabel_warna = _colour.weights_matching_cv2(cv2)
        except _colour.ColourMismatch as exc:
            print(f"    Info: jalur warna terfusi tidak dipakai ({exc}).")
            if KEEP_COLOUR:
                print("    Info: warna video sampul tidak dipertahankan.")
            if READBACK_COLOUR:
                print("    Info: read-back dijalankan pada jalur abu-abu (SVS_READBACK).")
    jaga_warna = bool(KEEP_COLOUR and tabel_warna)
    if jaga_warna:
        print("    Info: warna video sampul dipertahankan.")
    per_frame = (_batch.capacity_bits(1, out_h, out_w, num_ac_coeffs) if matriks is None
                 else _matrix.capacity_bits(1, out_h, out_w, _matrix.as_pair(matriks)[0]))
    # nothing can be embedded at delta <= 0 (:143-145) - unless a step table replaces delta
    usable = per_frame if delta_kuantisasi > 0 or tabel_langkah is not None else 0
    state = {"disisipkan": 0, "frame_num": 0, "first": None}
    if NEAREST:
        print("    Info: paritas koefisien dipaksa ke titik kisi terdekat (SVS_NEAREST).")
    terdekat = {"nearest": True} if NEAREST else {}                # no keyword at all when off: the calls stay what they were
    if MINMOVE:
        print("    Info: koefisien digeser sesedikit mungkin ke dalam sel keputusannya (SVS_MINMOVE).")
        terdekat["minmove"] = True
    if pilihan is not None:
        print(f"    Info: koefisien pembawa payload dipilih (SVS_COEFFS): {list(pilihan)}")
        terdekat = dict(terdekat, coeffs=pilihan)                  # the gray pipeline's keywords (the colour path is off)
    if kunci_dither is not None:
        print("    Info: kisi kuantisasi digeser dengan dither berkunci (SVS_DITHER_KEY).")
        terdekat = dict(terdekat, dither_key=kunci_dither)         # likewise
    if tabel_langkah is not None:
        print("    Info: langkah kuantisasi per koefisien dipakai (SVS_STEPS); DELTA tidak dipakai.")
        terdekat = dict(terdekat, steps=tabel_langkah)             # likewise
    if matriks is not None:
        print(f"    Info: penyisipan matriks dipakai (SVS_MATRIX): {_matrix.as_pair(matriks)[0]} bit per blok.")
        terdekat = dict(terdekat, matrix=matriks)                  # likewise
    readback_abu = READBACK or (READBACK_COLOUR and not tabel_warna)   # the gray pipeline's read-back
    rb_pipa = {"readback_keyed": True} if READBACK_KEYED else ({"readback": True} if readback_abu else {})
    if READBACK_STEPPED:
        rb_pipa = {"readback_stepped": True}
    if gerbang is not None:
        rb_pipa = {"readback_margin": gerbang}

    def lapor_readback(diperbaiki, tersisa, diperkuat=None, lemah=None):
        if diperkuat is None:
            print(f"    Read-back: {diperbaiki} blok diperbaiki, {tersisa} blok tidak dapat diperbaiki.")
        else:
            print(f"    Read-back: {diperbaiki} blok diperbaiki, {tersisa} blok tidak dapat diperbaiki, {diperkuat} blok diperkuat "
                  f"(margin >= {gerbang}), {lemah} blok tetap lemah.")
        if tersisa:
            print(f"    Warning: {tersisa} blok tidak terbaca kembali dengan benar; "
                  "payload kemungkinan gagal didekripsi.")

    def baca(n):
        """decode up to n frames, cropped; gray unless the fused colour path takes them as they are"""
        frames = []
        while len(frames) < n:
            ok, frame_bgr = cap.read()
            if not ok:
                break
            potong = frame_bgr[0:out_h, 0:out_w]
            frames.append(potong if tabel_warna else cv2.cvtColor(potong, cv2.COLOR_BGR2GRAY))
        return frames

    def tulis(gray_stack, stego_stack, stego_bgr=None):
        """encode one finished batch, one log line per frame as the reference prints them (:129)"""
        for k in range(len(stego_stack)):
            state["frame_num"] += 1
            bits_frame = min(usable, total_bits - state["disisipkan"])
            if state["frame_num"] == 1:
                # colours kept: B != G != R, the stego plane is the output's gray (cv2's table = the device's, checked above)
                stego0 = cv2.cvtColor(stego_bgr[0], cv2.COLOR_BGR2GRAY) if jaga_warna else stego_stack[0]
                state["first"] = (np.array(gray_stack[0]), np.array(stego0))
            writer.write(stego_bgr[k] if stego_bgr is not None else cv2.cvtColor(stego_stack[k], cv2.COLOR_GRAY2BGR))
            state["disisipkan"] += bits_frame
            print(f"    Frame {state['frame_num']}: {bits_frame} bits disisipkan. "
                  f"Total disisipkan: {state['disisipkan']}/{total_bits}")

    # frames that carry payload: frame k takes stream bits [k*cap, (k+1)*cap) (:116-128), so their number is known now
    carrying = -(-total_bits // usable) if usable else None        # None: every frame is entered, nothing is consumed
    habis = False
    if tabel_warna:
        # fused colour path (opt-in): synchronous batches through svs_embed_bgr
        sisa = carrying
        rb_total = [0, 0]
        while not habis and (sisa is None or sisa > 0):
            frames = baca(BATCH_FRAMES if sisa is None else min(BATCH_FRAMES, sisa))
            if not frames:
                habis = True
                break
            hasil = _batch.embed_bgr_frames(np.stack(frames), delta_kuantisasi, num_ac_coeffs, payload,
                                            bit_offset=state["disisipkan"], n_bits=total_bits - state["disisipkan"],
                                            weights=tabel_warna, keep_colour=jaga_warna,
                                            **({"readback": True} if READBACK_COLOUR else {}), **terdekat)
            stego_bgr, gray, used = hasil[:3]
            if READBACK_COLOUR:
                rb_total[0] += hasil[3].repaired
                rb_total[1] += hasil[3].unrepaired
            expect = min(len(frames) * usable, total_bits - state["disisipkan"])
            if used != expect:
                raise RuntimeError(f"embed kernel consumed {used} bits, expected {expect}")
            tulis(gray, stego_bgr[..., 0], stego_bgr)
            if sisa is not None:
                sisa -= len(frames)
        if READBACK_COLOUR:
            lapor_readback(*rb_total)
    else:
        # Overlapped staging: batch k+1 is decoded (feeder thread) while batch k is on the GPU (H2D copy,
        # kernel and D2H copy run asynchronously on the slot's stream) and batch k-1 is encoded (this thread); the payload is
        # uploaded once.
        per_batch = BATCH_FRAMES if carrying is None else max(1, min(BATCH_FRAMES, carrying))
        n_batches = PIPELINE_DEPTH if carrying is None else -(-carrying // per_batch)
        with FramePipeline(out_h, out_w, per_batch, delta_kuantisasi, num_ac_coeffs,
                           depth=max(1, min(PIPELINE_DEPTH, n_batches)), mode=_batch.host_level_mode(),
                           **_keyed(block_key=kunci_blok), **rb_pipa,
                           **terdekat) as pipe:
            pipe.set_payload(payload)
            rencana = {"sisa": carrying}

            def isi(slot):
                """decode the next batch straight into the slot's pinned input (feeder thread)"""
                mau = per_batch if rencana["sisa"] is None else min(per_batch, rencana["sisa"])
                masukan, n = pipe.input(slot), 0
                while n < mau:
                    ok, frame_bgr = cap.read()
                    if not ok:
                        break
                    masukan[n] = cv2.cvtColor(frame_bgr[0:out_h, 0:out_w], cv2.COLOR_BGR2GRAY)
                    n += 1
                if rencana["sisa"] is not None:
                    rencana["sisa"] -= n
                return n

            def kirim(slot, k, n):
                offset = k * per_batch * usable
                used = pipe.submit_embed(slot, n, bit_offset=min(offset, total_bits),
                                         **_keyed(kunci_blok, kunci_dither, first_frame=k * per_batch))
                return used, min(n * usable, max(0, total_bits - offset))

            with SlotFeeder(pipe, isi, kirim) as feeder:
                for slot, k, n, (used, expect) in feeder:
                    if used != expect:
                        raise RuntimeError(f"embed kernel consumed {used} bits, expected {expect}")
                    tulis(pipe.input(slot)[:n], pipe.embed_result(slot))
                    feeder.release(slot)
            if rb_pipa:
                lapor_readback(*(pipe.margin_counts() if gerbang is not None else pipe.readback_counts()))
    disisipkan = state["disisipkan"]
    selesai = usable > 0 and disisipkan >= total_bits
    if selesai:
        print("    Semua payload (SHA3-ECC-AES) berhasil disisipkan!")
        for frame_bgr in read_ahead(cap.read):                         # remaining frames: copied, in colour (:134-139);
            writer.write(frame_bgr[0:out_h, 0:out_w])                  # decoded on a thread while this one encodes
    else:
        print(f"    Warning: Video selesai sebelum semua payload ({total_bits} bits) disisipkan.")
    first_gray, first_stego = state["first"] if state["first"] else (None, None)
    cap.release()
    writer.release()
    if selesai:
        print(f"  Proses embedding (SHA3-ECC-AES) selesai. Video output: '{path_out}'.")
        return True, first_gray, first_stego
    print("  Proses embedding (SHA3-ECC-AES) selesai, namun TIDAK semua data berhasil disisipkan.")
    return False, None, None


if __name__ == "__main__":
    # same hard-coded demo as the reference's __main__ (embed_process.py:155-217)
    input_dir, output_dir = "media/input", "media/output"
    os.makedirs(output_dir, exist_ok=True)
    video_in = os.path.join(input_dir, "cover.mp4")
    gambar = os.path.join(input_dir, "ini_adalah_rahasia_grayscale.png")
    video_out = os.path.join(output_dir, "stego_video_final")
    DELTA, N_AC = 20, 10
    siap = persiapkan_file_input(input_dir, video_in, gambar)
    priv, pub_bytes = setup_kunci_ecc()
    if siap and pub_bytes:
        ok, g0, s0 = embed_gambar_ke_video_final(video_in, gambar, video_out, DELTA, N_AC, pub_bytes)
        if ok and g0 is not None:
            print(f"  PSNR Frame Pertama (Asli vs. Stego): {_cv2().PSNR(g0, s0):.2f} dB")
        print("PROSES EMBEDDING " + ("BERHASIL" if ok else "GAGAL"))
