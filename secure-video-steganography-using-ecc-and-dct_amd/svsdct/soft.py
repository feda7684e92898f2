"""Reading and combining the bytes of the soft-decision extraction (svs_soft_extract, include/svsdct.h;
batch.extract_soft_frames).  NumPy only: nothing here loads the library or touches the GPU.

One byte per capacity bit, in stream order: bit 7 is the hard bit, bits 0..6 are m, the distance of the payload coefficient
from the nearest decision boundary of its quantiser cell in units of delta / 254 - 127 on the lattice point, 0 on the
boundary.  m is a DISTANCE, not a probability: what it says about the chance of a bit error depends on the disturbance
between sender and receiver, which nobody here knows.

A sender that wants a payload to survive a lost bit tiles it - tile(): copy after copy through the stream, the last one cut
where the capacity ends - and embeds the tiled stream as any other (batch.embed_repeated_frames); the receiver extracts soft
bytes and folds them with combine(), or has the device fold them in the extract launch (svs_soft_vote, batch.extract_vote_frames)
and gets the tally of tally() back: `period` integers whose signs are combine()'s bits.

A receiver that only asks which frames sit on the lattice, or a sender that asks for the lowest reliability of each frame, needs
no byte at all: svs_soft_histogram (batch.extract_histogram_frames) returns 256 counts a frame, the array of byte_histogram();
margins() and lattice_share() read it.
"""
from __future__ import annotations

import numpy as np


def _soft(soft) -> np.ndarray:
    a = np.asarray(soft)
    if a.dtype != np.uint8 or a.ndim != 1:
        raise TypeError("soft must be a one-dimensional uint8 array (one byte per capacity bit)")
    return a


def hard_bits(soft) -> np.ndarray:
    """the hard bits, uint8 0 / 1 per byte: numpy.packbits of them is what the matching extract call returns"""
    return _soft(soft) >> 7


def reliability(soft) -> np.ndarray:
    """m per byte, uint8 in 0..127"""
    return _soft(soft) & np.uint8(127)


def combine(soft, period: int):
    """Soft vote over the copies of a tiled payload of `period` bits: byte j, j + period, j + 2 period, .. are copies of
    payload bit j, a last partial copy counting where it reaches.  Every copy votes (2 b - 1) (2 m + 1) - its hard bit, weighted
    by an odd number so that no single byte abstains - and
        score[j] = sum of the votes,    bit[j] = score[j] > 0,    a zero score takes copy 0's bit.
    Returns (bits uint8 [period], score int32 [period]).  period must be in 1 .. len(soft)."""
    a = _soft(soft)
    period = int(period)
    if not 1 <= period <= a.size:
        raise ValueError(f"period {period} outside 1 .. {a.size}")
    votes = (2 * (a >> 7).astype(np.int32) - 1) * (2 * (a & 127).astype(np.int32) + 1)
    copies = -(-a.size // period)
    padded = np.zeros(copies * period, np.int32)
    padded[: a.size] = votes
    score = padded.reshape(copies, period).sum(axis=0, dtype=np.int32)
    bits = np.where(score != 0, score > 0, a[:period] >> 7).astype(np.uint8)
    return bits, score


def tile(bits, n_bits: int) -> np.ndarray:
    """the payload repeated to n_bits stream bits, the last copy cut: uint8 0 / 1.  ValueError for an empty payload"""
    b = np.asarray(bits, np.uint8).reshape(-1)
    n_bits = int(n_bits)
    if b.size == 0:
        raise ValueError("an empty payload cannot be tiled")
    if n_bits < 0:
        raise ValueError("n_bits is negative")
    return np.resize(b, n_bits)


def tally(soft, period: int, stream_bit0: int = 0) -> np.ndarray:
    """The tally of the fused vote (svs_soft_vote, include/svsdct.h) on soft bytes: byte i has stream position
    p = stream_bit0 + i and adds 2 (2 b - 1) (2 m + 1) to entry p mod period, and (2 b - 1) more where p < period - copy 0
    breaks ties, so an entry that copy 0 has reached is odd and never 0.  Tallies of consecutive pieces of a stream, each at its
    own stream_bit0, add up to the tally of the whole.  period may exceed len(soft).  int32 [period]."""
    a = _soft(soft)
    period, stream_bit0 = int(period), int(stream_bit0)
    if period < 1 or stream_bit0 < 0:
        raise ValueError("period must be at least 1 and stream_bit0 at least 0")
    sign = 2 * (a >> 7).astype(np.int64) - 1
    head = np.arange(a.size, dtype=np.int64) < max(period - stream_bit0, 0)             # p < period: the bits of copy 0
    votes = 2 * sign * (2 * (a & 127).astype(np.int64) + 1) + sign * head
    base = stream_bit0 % period                                                         # byte i sits at residue (base + i) mod period
    rows = -(-(base + a.size) // period)
    padded = np.zeros(max(rows, 1) * period, np.int64)
    padded[base: base + a.size] = votes
    out = padded.reshape(-1, period).sum(axis=0)
    if np.abs(out).max() >= 1 << 31:
        raise OverflowError("a tally entry leaves int32")
    return out.astype(np.int32)


def tally_bits(tally) -> np.ndarray:
    """the decoded payload bits of a tally, uint8 0 / 1: entry > 0"""
    return (np.asarray(tally) > 0).astype(np.uint8)


def margin_histogram(soft, n_frames: int) -> np.ndarray:
    """int64 [n_frames, 128]: how many bytes of each frame have each m.  The stream is the frames' bytes in order, equally many
    per frame.  A frame whose payload coefficients sit on the lattice - stego read with the right dither, or without one -
    has its mass near 127; a never-embedded frame, or dithered stego read without the key, is flat."""
    a = _soft(soft)
    n_frames = int(n_frames)
    if n_frames < 1 or a.size % n_frames:
        raise ValueError(f"{a.size} bytes are not {n_frames} frames of equal capacity")
    m = (a & 127).reshape(n_frames, -1).astype(np.int64)
    hist = np.zeros((n_frames, 128), np.int64)
    np.add.at(hist, (np.repeat(np.arange(n_frames), m.shape[1]), m.ravel()), 1)
    return hist


def byte_histogram(soft, n_frames: int) -> np.ndarray:
    """int64 [n_frames, 256]: how many bytes of each frame have each value - the format of svs_soft_histogram
    (include/svsdct.h) on soft bytes.  The stream is the frames' bytes in order, equally many per frame; row f sums to that
    number, row[128:] counts the frame's hard ones."""
    a = _soft(soft)
    n_frames = int(n_frames)
    if n_frames < 1 or a.size % n_frames:
        raise ValueError(f"{a.size} bytes are not {n_frames} frames of equal capacity")
    per = a.size // n_frames
    at = np.repeat(np.arange(n_frames, dtype=np.int64), per) * 256 + a
    return np.bincount(at, minlength=256 * n_frames).astype(np.int64).reshape(n_frames, 256)


def _hist(hist) -> np.ndarray:
    h = np.asarray(hist)
    if h.ndim != 2 or h.shape[1] != 256 or h.dtype.kind not in "iu":
        raise TypeError("hist must be an integer array [n_frames, 256] (byte_histogram, svs_soft_histogram)")
    return h.astype(np.int64)


def margins(hist) -> np.ndarray:
    """int64 [n_frames, 128]: the counts per m of a byte histogram, both hard bits together - margin_histogram of the bytes"""
    h = _hist(hist)
    return h[:, :128] + h[:, 128:]


def lattice_share(hist, m_min: int = 64) -> np.ndarray:
    """float64 per frame: the share of a frame's bytes with m >= m_min.  1.0 for stego read without a dither or with its key,
    about a half for a never-embedded frame and for dithered stego read without the key; a frame without a byte gives nan.
    A distance statistic, not a detector: every block of the frame is counted, payload or not."""
    m_min = int(m_min)
    if not 0 <= m_min <= 128:
        raise ValueError("m_min outside 0 .. 128")
    m = margins(hist)
    total = m.sum(axis=1).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return m[:, m_min:].sum(axis=1) / total
