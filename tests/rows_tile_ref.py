"""NumPy restatement of cm3_rows_tile's row formula (include/cm3_amd.h, cm3_tile_col): destination row r <- source row f(r), and what
each kind writes per element.  Lives under tests/: the product has no CPU path (tests/test_abi.py)."""
import numpy as np
import torch

TILE_COPY, TILE_F32_TO_F64, TILE_ONEHOT_I64, TILE_ONEHOT_F64, TILE_EYE_F64, TILE_NOT_I64 = range(6)
NP_DTYPE = {torch.float64: np.float64, torch.float32: np.float32, torch.int64: np.int64, torch.int32: np.int32, torch.bool: np.bool_,
            torch.uint8: np.uint8}


def source_rows(n_rows, terms=None, others=None):
    """f(r) for r in range(n_rows)"""
    r = np.arange(int(n_rows), dtype=np.int64)
    if others is not None:
        N, divq, divn = others
        k, n = r % (N - 1), (r // divn) % N
        return (r // divq) * N + k + (k >= n)
    s = np.zeros_like(r)
    for div, mod, mul in terms:
        q = r // div
        if mod:
            q = q % mod
        s = s + q * mul
    return s


def tile(spec, src):
    """The array one TileSpec (cm3_amd.batch) yields from its source column `src` (a NumPy array; its leading dimensions are flattened
    into rows of spec.epr elements, one element per row for the one-hot kinds)."""
    f = source_rows(spec.rows, spec.terms, spec.others)
    e = np.arange(spec.epr)
    if spec.kind == TILE_COPY:
        out = np.ascontiguousarray(src).reshape(-1, spec.epr)[f]
    elif spec.kind == TILE_F32_TO_F64:
        out = np.ascontiguousarray(src).reshape(-1, spec.epr)[f].astype(np.float64)
    elif spec.kind in (TILE_ONEHOT_I64, TILE_ONEHOT_F64):
        out = (np.asarray(src).reshape(-1)[f][:, None] == e[None, :]).astype(np.int64 if spec.kind == TILE_ONEHOT_I64 else np.float64)
    elif spec.kind == TILE_EYE_F64:
        out = ((np.arange(spec.rows) % spec.epr)[:, None] == e[None, :]).astype(np.float64)
    elif spec.kind == TILE_NOT_I64:
        out = 1 - (np.ascontiguousarray(src).reshape(-1, spec.epr)[f] != 0).astype(np.int64)
    else:
        raise ValueError("unknown kind %r" % (spec.kind,))
    out = out.astype(NP_DTYPE[spec.dtype])
    return out.reshape(spec.shape if spec.shape is not None else (spec.rows, spec.epr))


def static_feeds(cols, specs):
    """name -> CPU torch tensor for every spec, from a dict of columns (NumPy arrays or CPU tensors) keyed as the specs' sources."""
    out = {}
    for s in specs:
        src = None if s.src is None else cols[s.src]
        if torch.is_tensor(src):
            src = src.numpy()
        out[s.name] = torch.from_numpy(np.ascontiguousarray(tile(s, src)))
    return out
