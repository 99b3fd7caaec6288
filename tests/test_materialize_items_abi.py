"""CPU tests of the materialize-items entry points (include/lsmgpu.h, section
"materialize items"): the three symbols are exported and listed, the workspace size is
monotone and non-zero for no items, and argument validation answers LSM_BAD_ARG before
any HIP call (fake, never dereferenced device addresses; no GPU here)."""
import ctypes as C

import pytest

BAD_ARG = 10
NAMES = ("lsm_materialize_items_workspace_size", "lsm_materialize_items_plan", "lsm_materialize_items")
REQUIRED_FIELDS = ("key_off", "key_len", "prefix_len", "val_off", "val_len", "seqno", "vtype")
N_ITEMS = 1000


@pytest.fixture(scope="module")
def L():
    import lsmgpu
    if not lsmgpu.LIB_PATH.exists():
        lsmgpu.build()
    return lsmgpu


def _parsed(L, missing=None):
    ps = L.LsmParsed()
    for k, f in enumerate(REQUIRED_FIELDS):
        setattr(ps, f, None if f == missing else 0x100000 * (k + 1))
    return ps


def _addr(k):
    return C.c_void_p(0x10000000 + 0x1000 * k)


def _plan_args(L, ps, **override):
    """Every argument of lsm_materialize_items_plan, valid but for the overrides."""
    a = {"d_blocks": _addr(1), "d_block_off": _addr(2), "n_blocks": 4, "d_n_blocks": None, "d_item_start": _addr(3),
         "d_status": _addr(4), "d_parsed": C.byref(ps), "n_items": N_ITEMS, "d_base": None, "d_out_key_off": _addr(5),
         "d_out_val_off": _addr(6), "out_item_cap": N_ITEMS, "d_end": _addr(7), "d_result": _addr(8),
         "d_workspace": _addr(9), "workspace_bytes": L.lib().lsm_materialize_items_workspace_size(N_ITEMS),
         "stream": None}
    a.update(override)
    return tuple(a.values())


def _gather_args(L, ps, **override):
    a = {"d_blocks": _addr(1), "d_block_off": _addr(2), "n_blocks": 4, "d_n_blocks": None, "d_item_start": _addr(3),
         "d_status": _addr(4), "d_parsed": C.byref(ps), "n_items": N_ITEMS, "d_base": None, "d_end": _addr(7),
         "d_out_key_off": _addr(5), "d_out_val_off": _addr(6), "d_out_keys": _addr(10), "key_cap": 1 << 20,
         "d_out_vals": _addr(11), "val_cap": 1 << 20, "d_out_seqno": _addr(12), "d_out_vtype": _addr(13),
         "out_item_cap": N_ITEMS, "d_result": _addr(8), "stream": None}
    a.update(override)
    return tuple(a.values())


def test_symbols_exported_and_listed(L):
    lib = L.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in L.EXPORTED_SYMBOLS
    header = (L.HERE.parent / "include" / "lsmgpu.h").read_text()
    for name in NAMES:
        assert name + "(" in header
    assert lib.lsm_abi_version() == 7  # additions only


def test_workspace_size_monotone_and_nonzero(L):
    size = L.lib().lsm_materialize_items_workspace_size
    sizes = [size(n) for n in (0, 1, 63, 64, 65, 2047, 2048, 2049, 1 << 20, 1 << 26, 1 << 32)]
    assert sizes[0] > 0
    assert sizes == sorted(sizes)
    assert sizes[-1] >= 8 * (1 << 32)  # two u32 lengths per row


@pytest.mark.parametrize("null", ["d_blocks", "d_item_start", "d_status", "d_parsed", "d_end", "d_result"])
def test_plan_null_argument_is_bad_arg(L, null):
    ps = _parsed(L)
    assert L.lib().lsm_materialize_items_plan(*_plan_args(L, ps, **{null: None})) == BAD_ARG


@pytest.mark.parametrize("null", ["d_blocks", "d_item_start", "d_status", "d_parsed", "d_end", "d_result"])
def test_gather_null_argument_is_bad_arg(L, null):
    ps = _parsed(L)
    assert L.lib().lsm_materialize_items(*_gather_args(L, ps, **{null: None})) == BAD_ARG


@pytest.mark.parametrize("field", REQUIRED_FIELDS)
def test_missing_parsed_field_is_bad_arg(L, field):
    ps = _parsed(L, missing=field)
    assert L.lib().lsm_materialize_items_plan(*_plan_args(L, ps)) == BAD_ARG
    assert L.lib().lsm_materialize_items(*_gather_args(L, ps)) == BAD_ARG


def test_workspace_too_small_is_bad_arg(L):
    ps = _parsed(L)
    need = L.lib().lsm_materialize_items_workspace_size(N_ITEMS)
    assert L.lib().lsm_materialize_items_plan(*_plan_args(L, ps, workspace_bytes=need - 1)) == BAD_ARG
    assert L.lib().lsm_materialize_items_plan(*_plan_args(L, ps, d_workspace=None)) == BAD_ARG
    # the same for no items: the cursor record still lives in the workspace
    need0 = L.lib().lsm_materialize_items_workspace_size(0)
    assert L.lib().lsm_materialize_items_plan(*_plan_args(L, ps, n_items=0, workspace_bytes=need0 - 1)) == BAD_ARG
