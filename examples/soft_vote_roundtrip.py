#!/usr/bin/env python3
"""Repetition by tiling, decoded by the fused soft vote: a framed payload (svsdct.framing) is written copy after copy through the
stream of a clip of synthetic noise (batch.embed_repeated_frames), the stego is disturbed with uniform pixel noise, and the
receiver has the device fold the copies by their reliabilities (batch.extract_vote_frames: `period` integers come back, no
soft byte is written) before it parses the header.  The same vote on the soft bytes (batch.extract_soft_frames,
svsdct.soft.combine) is run beside it: the bits are the same.  The sender tiles the bits, the receiver knows the period.
The clip is sized for --copies copies and then filled to its capacity (copies=None), the last copy cut: the fused vote reads
every capacity bit of the frames it is given, so bits the sender left unembedded would vote as noise.

    python examples/soft_vote_roundtrip.py [--noise 5] [--copies 3] [--n-ac 10] [--delta 20]

At the defaults a single copy has bit errors and the vote has none; from about +-8 on the vote leaves a few (README.md has the
table), and the header - which has no error correction of its own - no longer parses.  The cover is noise in [64, 192): pixels
that clip at 0 or 255 lose bits before any disturbance (that is what read-back repairs).
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "secure-video-steganography-using-ecc-and-dct_amd"))
import numpy as np  # noqa: E402

from svsdct import batch, framing, soft  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--noise", type=int, default=5, help="amplitude a of the uniform integer pixel noise in [-a, a]")
ap.add_argument("--copies", type=int, default=3, help="the clip is sized to hold at least this many copies, and then filled")
ap.add_argument("--n-ac", type=int, default=10)
ap.add_argument("--delta", type=float, default=20)
a = ap.parse_args()

h, w = 360, 640
secret = (np.add.outer(np.arange(32), np.arange(32)) * 4 % 256).astype(np.uint8)       # a 32x32 gray "image"
payload = framing.build_payload_bits(32, 32, b"\x02" + bytes(32), bytes(16), bytes(32), bytes(12), bytes(16),
                                     secret.tobytes())                                   # unencrypted, for the demo
per_frame = batch.capacity_bits(1, h, w, a.n_ac)
frames = -(-a.copies * payload.size // per_frame)
rng = np.random.default_rng(2)
clip = rng.integers(64, 192, (frames, h, w)).astype(np.uint8)
stego, used, period = batch.embed_repeated_frames(clip, a.delta, a.n_ac, payload)            # soft.tile + embed_frames
print(f"payload {period} bits, {frames} frames of {per_frame} bits: {used / period:.2f} copies")
disturbed = np.clip(stego.astype(np.int64) + rng.integers(-a.noise, a.noise + 1, stego.shape), 0, 255).astype(np.uint8)
bytes_, n = batch.extract_soft_frames(disturbed, a.delta, a.n_ac)
assert used == n                                                                         # the clip is full
hard = soft.hard_bits(bytes_)
voted, score = soft.combine(bytes_, period)
fused, tally = batch.extract_vote_frames(disturbed, a.delta, a.n_ac, period)             # the same vote, folded on the device
print("the fused vote's bits equal soft.combine's:", bool(np.array_equal(fused, voted)),
      "| its tally is soft.tally of the soft bytes:", bool(np.array_equal(tally, soft.tally(bytes_, period))))
print("bit errors of each whole copy alone:", [int((hard[k * period:(k + 1) * period] != payload).sum()) for k in range(used // period)],
      "| after the soft vote:", int((voted != payload).sum()), "| smallest |score|:", int(np.abs(score).min()))
try:
    hdr = framing.parse_header(voted)
    got = np.packbits(voted[hdr.bits:hdr.bits + 8 * hdr.ciphertext_len])
    print("header:", hdr.width, "x", hdr.height, "ciphertext bytes", hdr.ciphertext_len, "| image recovered:",
          bool(got.size == secret.size and np.array_equal(got.reshape(secret.shape), secret)))
except ValueError as exc:                                                                # too much noise for three copies
    print("the header does not parse:", exc)
hist = soft.margin_histogram(batch.extract_soft_frames(stego, a.delta, a.n_ac)[0], frames)
print("share of coefficients within delta/4 of the lattice, undisturbed stego, per frame:",
      [round(float(hist[k, 64:].sum() / hist[k].sum()), 3) for k in range(frames)])
