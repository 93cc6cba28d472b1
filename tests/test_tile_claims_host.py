"""Host side of the tile-claim switches, without a GPU: the workgroup cap's argument clause and the place of
NrNeusArgs.serial_order (appended, so callers built against the shorter struct keep every other offset)."""
from neurecon_amd import _lib as L

ARG = -1


def test_workgroup_cap_rejects_a_negative_cap():
    lib = L.lib()
    assert lib.nr_set_workgroup_cap(-1) == ARG
    assert b'nr_set_workgroup_cap: the cap must be >= 0' in lib.nr_last_error()
    try:
        assert lib.nr_set_workgroup_cap(3) == 0
    finally:
        assert lib.nr_set_workgroup_cap(0) == 0


def test_serial_order_is_the_last_field_and_defaults_to_off():
    name, _ = L.NrNeusArgs._fields_[-1]
    assert name == 'serial_order'
    assert L.NrNeusArgs._fields_[-2][0] == 'fold_packed'
    assert L.NrNeusArgs().serial_order == 0
