#!/usr/bin/env python3
"""What of a stego clip survives an 8x8 intra codec: a payload is tiled over three frames of synthetic noise
(batch.embed_repeated_frames: one copy per frame), the stego goes through the requantisation channel
(batch.requantise_frames: the luminance path of JPEG / MJPEG on the embed's grid, include/svsdct.h) at a list of qualities, and
for each quality the receiver's numbers are printed: the bit errors of each copy alone, those of the fused soft vote
(batch.extract_vote_frames) and, from the fused per-frame histograms, the share of coefficients still within delta / 4 of the
lattice (soft.lattice_share).

    python examples/recompression_survival.py [--delta 20] [--n-ac 10] [--rule reference|nearest|minmove]
                                              [--zigzag FIRST] [--qualities 100,95,90,85,75,50]

Everything runs on the GPU through the library.  The channel is a format, so the numbers equal those of the CPU model
(tests/channel_lib.py) for the same seed - at the defaults the reference-rule row of README.md's table: no error down to
quality 85, and at 75 copies that fail together, which the soft vote mends in part.  The model is luminance only, grid-aligned,
without chroma subsampling, motion prediction or deblocking.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "secure-video-steganography-using-ecc-and-dct_amd"))
import numpy as np  # noqa: E402

from svsdct import batch, soft  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--delta", type=float, default=20)
ap.add_argument("--n-ac", type=int, default=10, help="payload coefficients per block")
ap.add_argument("--rule", choices=("reference", "nearest", "minmove"), default="reference")
ap.add_argument("--zigzag", type=int, default=0, metavar="FIRST",
                help="put the payload on zig-zag scan positions FIRST .. FIRST + n_ac - 1 instead of the row-major prefix")
ap.add_argument("--qualities", default="100,95,90,85,75,50")
a = ap.parse_args()

f, h, w = 3, 96, 160
rng = np.random.default_rng(5)
cover = rng.integers(64, 192, (f, h, w)).astype(np.uint8)                     # no pixel clips at 0 or 255 before the channel
payload = rng.integers(0, 2, batch.capacity_bits(1, h, w, a.n_ac)).astype(np.uint8)
kw = dict(coeffs=f"zigzag:{a.zigzag}") if a.zigzag else {}
stego, used, period = batch.embed_repeated_frames(cover, a.delta, a.n_ac, payload, mode="exact", nearest=a.rule == "nearest",
                                                  minmove=a.rule == "minmove", **kw)
assert (used, period) == (f * payload.size, payload.size)
print(f"{f} frames of {w}x{h}, one copy of {period} bits per frame, delta = {a.delta:g}, n = {a.n_ac}, {a.rule} rule"
      + (f", zig-zag from {a.zigzag}" if a.zigzag else ""))
print("quality | errors of each copy alone | fused soft vote | lattice share per frame")
for quality in (int(q) for q in a.qualities.split(",")):
    seen = batch.requantise_frames(stego, quality)
    bytes_, n = batch.extract_soft_frames(seen, a.delta, a.n_ac, **kw)
    voted, _ = batch.extract_vote_frames(seen, a.delta, a.n_ac, period, **kw)
    hist, _ = batch.extract_histogram_frames(seen, a.delta, a.n_ac, **kw)
    single = [int((soft.hard_bits(bytes_[k * period:(k + 1) * period]) != payload).sum()) for k in range(f)]
    print(f"{quality:7d} | {' / '.join(str(e) for e in single):25s} | {int((voted != payload).sum()):15d} | "
          + " ".join(f"{s:.3f}" for s in soft.lattice_share(hist)))
