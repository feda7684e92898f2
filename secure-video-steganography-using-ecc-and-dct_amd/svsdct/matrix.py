"""Matrix embedding (include/svsdct.h, svs_matrix_embed* / svs_matrix_extract*): a block of 2^k - 1 payload coefficients carries k
message bits as the Hamming syndrome of their parities, so the sender flips at most one parity a block - or, with the pair
search, the cheaper of one flip and a pair.  A stepped call: it goes together with steps= (svsdct/steps.py; steps.uniform(20) for
one delta) and pays off under minmove=True.  The calls themselves run on the GPU (svsdct/batch.py, matrix=); the host model of
the format lives with the tests (tests/matrix_lib.py)."""
from __future__ import annotations

import os

import numpy as np

from .native import Matrix

K_MAX = 6
PAIR_K_MAX = 5      # the pair search keeps 2 (2^k - 1) floats a lane in LDS: k = 6 exceeds what a launch may request


def as_pair(matrix) -> tuple[int, int]:
    """matrix= of the batch calls -> (k, search): an int k in 1..6 (the syndrome's single flip) or (k, "pair") (the cheapest of
    one flip or a pair, k <= 5); (k, "single") is k"""
    search = "single"
    if isinstance(matrix, (tuple, list)):
        if len(matrix) != 2:
            raise ValueError('matrix is k or (k, "pair")')
        matrix, search = matrix
    if isinstance(matrix, bool) or not isinstance(matrix, (int, np.integer)) or not 1 <= matrix <= K_MAX:
        raise ValueError(f"matrix k {matrix!r} is not an int in 1..{K_MAX}")
    if search not in ("single", "pair"):
        raise ValueError(f'matrix search {search!r} is neither "single" nor "pair"')
    if search == "pair" and matrix > PAIR_K_MAX:
        raise ValueError(f"the pair search takes k <= {PAIR_K_MAX}")
    return int(matrix), int(search == "pair")


def slots(k: int) -> int:
    """the payload coefficients a block needs for k bits: the size of the selection (or n_ac) of a matrix call"""
    return (1 << int(k)) - 1


def matrix_struct(k: int, search: int = 0) -> Matrix:
    """struct svs_matrix"""
    return Matrix(int(k), int(search), (Matrix._fields_[2][1])(0, 0))


def capacity_bits(n_frames: int, height: int, width: int, k: int) -> int:
    """blocks * k - svs_matrix_capacity_bits, in integers"""
    if not 1 <= int(k) <= K_MAX or n_frames <= 0 or height <= 0 or width <= 0:
        return 0
    return int(n_frames) * (int(height) // 8) * (int(width) // 8) * int(k)


def parse(spec: str):
    """`k` or `k:pair` -> the value matrix= takes"""
    head, _, tail = spec.strip().partition(":")
    try:
        k = int(head)
    except ValueError:
        raise ValueError(f"SVS_MATRIX {spec!r} is neither k nor k:pair") from None
    if tail not in ("", "pair", "single"):
        raise ValueError(f"SVS_MATRIX {spec!r} is neither k nor k:pair")
    value = (k, "pair") if tail == "pair" else k
    as_pair(value)
    return value


def from_env(environ=None):
    """the value SVS_MATRIX names (parse), None when the variable is unset or empty"""
    spec = (os.environ if environ is None else environ).get("SVS_MATRIX", "")
    return parse(spec) if spec.strip() else None
