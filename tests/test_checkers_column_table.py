"""CPU: the 16 Checkers transition columns are ONE list -- the fields of both ctypes column structs, CHECKERS_ORDER and
CheckersRollout.ORDER -- and the column specs made from the per-record description have the row sizes the compact ring quotes."""
import types

import torch


def test_one_name_tuple_is_the_field_order_of_both_structs_and_the_order_of_the_columns():
    from cm3_amd import _lib
    from cm3_amd.rollout import CHECKERS_ORDER, CheckersRollout
    names = _lib.CHECKERS_COLUMNS
    assert len(names) == len(set(names)) == 16 and names == tuple(n for n, _ in _lib.CHECKERS_COLUMN_RECORDS)
    for cls in (_lib.CheckersTransitionCols, _lib.CheckersCompactCols):
        assert tuple(n for n, _ in cls._fields_) == names + ("ring_start", "ring_size"), cls
    assert CHECKERS_ORDER is names and CheckersRollout.ORDER is names


def _row_bytes(specs):
    return sum(torch.empty(shape, dtype=dt).numel() * torch.empty((), dtype=dt).element_size() for shape, dt in specs.values())


def test_specs_from_the_record_description_have_the_row_bytes_of_the_reference_geometry():
    from cm3_amd.rollout import CHECKERS_ORDER, CheckersRollout, compact_specs
    ro = CheckersRollout.__new__(CheckersRollout)             # a stub env: 3 x 8 board, n_obs 2 (K = 5), N = 2
    ro.env = types.SimpleNamespace(n=2, R=3, C=8, K=5, Lo=2)
    wide, compact = ro.column_specs(), ro.compact_column_specs()
    assert tuple(wide) == tuple(compact) == CHECKERS_ORDER
    assert _row_bytes(wide) == 3657 and _row_bytes(compact) == 707
    assert compact == compact_specs(wide)
    assert wide["goals"] == ((2, 2), torch.int64) and compact["goals"] == ((2,), torch.uint8)
    assert wide["actions_prev"] == wide["actions"] == compact["actions_prev"] == ((2,), torch.int32)
    for name in ("grid", "vec", "obs_others", "obs_self_t", "obs_self_v"):
        assert wide["next_" + name] == wide[name] and compact["next_" + name] == compact[name], name
