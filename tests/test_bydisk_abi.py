"""The per-UAV attribution symbols (include/maxcover.h mac_area_by_disk_*) without a GPU: they are
exported and bound, and a null context is refused before anything touches a device."""
import ctypes

import numpy as np
import pytest

SYMBOLS = ("mac_area_by_disk_f64", "mac_area_by_disk_batch_f64", "mac_area_by_disk_dev_f64")


def test_symbols_in_exports(pkg):
    L = pkg.load_library()
    for name in SYMBOLS:
        assert name in pkg._lib.EXPORTS
        assert getattr(L, name).restype is ctypes.c_int32
    for meth in ("area_by_disk", "area_by_disk_batch", "area_by_disk_dev"):
        assert callable(getattr(pkg.Context, meth))
    assert callable(pkg.AreaCoverageCalculation.calculateAreaByDisk)


@pytest.mark.parametrize("name", SYMBOLS)
def test_null_context_is_invalid(pkg, name):
    L = pkg.load_library()
    dp = ctypes.POINTER(ctypes.c_double)
    c = np.array([1.0, 2.0, 3.0])
    owned, excl, area = np.full(1, -1.0), np.full(1, -1.0), np.full(1, -1.0)
    if name == "mac_area_by_disk_f64":
        rc = L.mac_area_by_disk_f64(None, c.ctypes.data_as(dp), 3, owned.ctypes.data_as(dp),
                                    excl.ctypes.data_as(dp), area.ctypes.data_as(dp))
    elif name == "mac_area_by_disk_batch_f64":
        rc = L.mac_area_by_disk_batch_f64(None, c.ctypes.data_as(dp), 3, 1, owned.ctypes.data_as(dp),
                                          excl.ctypes.data_as(dp), area.ctypes.data_as(dp))
    else:
        rc = L.mac_area_by_disk_dev_f64(None, None, 3, 1, None, None, None, None)
    assert rc == pkg._lib.MAC_E_INVAL
    assert b"null context" in L.mac_last_error()
    assert owned[0] == excl[0] == area[0] == -1.0   # nothing written
