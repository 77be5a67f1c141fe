"""TEST INFRASTRUCTURE ONLY -- NumPy restatement of the draw of the particle actor over transition rows
(cm3_actor_particle_rows_f32; rows_uniform in cm3_amd/csrc/actor_common.h), from the primitives of oracle/philox.py.

A sampled batch has no env, episode or step behind it, so the uniform of row r is keyed by the row alone:
    counter (row id lo, row id hi, draw, PURPOSE_ROWS), key = seed, word .x, u = float32((word + 0.5) * 2^-32)
with row id = row_id_base + r (64 bit) and draw the 32-bit counter the caller advances once per launch.  PURPOSE_ROWS is bit 28 of
counter word 3: the action (0), exploration (bit 29), policy (bit 30) and reset (bit 31) streams put at most `call << 24` with
call <= 4 or a small call index below their purpose bit, so none of them can produce this word.
"""
import numpy as np

from oracle import philox

PURPOSE_ROWS = 0x10000000


def rows_words(seed, row_ids, draw):
    """uint32 [R]: word .x of the Philox block of every row id."""
    lo, hi = philox._split(np.asarray(row_ids, dtype=np.uint64))
    return philox.philox4x32_10(lo, hi, np.uint64(int(draw) & 0xFFFFFFFF), np.uint64(PURPOSE_ROWS),
                                seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]


def rows_uniforms(seed, n_rows, draw, row_id_base=0):
    """float32 [n_rows]: the uniforms the rows kernel draws for rows row_id_base .. row_id_base + n_rows - 1 of launch `draw`."""
    ids = (np.arange(n_rows, dtype=np.uint64) + np.uint64(int(row_id_base) & 0xFFFFFFFFFFFFFFFF))
    return philox.u01(rows_words(seed, ids, draw)).astype(np.float32)
