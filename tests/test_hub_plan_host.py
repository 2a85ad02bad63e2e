"""The hub plan as one value on the host: ``_native.HubPlan`` carries the threshold and chunk it
was computed for, and ``_csr`` / ``_hub_args`` / ``_hub6`` take them from the plan, never from the
module.  The structs only need ``data_ptr()``, which CPU tensors have.  No GPU needed."""
import gc
import weakref

import pytest
import torch

from pytorch_geometric_amd import _native
from pytorch_geometric_amd._lib import SpmmArgs

OWN, OTHER = (64, 48), (9, 5)      # the plan's pair; what the module says at launch time


@pytest.fixture
def other_module_pair(monkeypatch):
    monkeypatch.setattr(_native, 'HUB_THRESHOLD', OTHER[0])
    monkeypatch.setattr(_native, 'HUB_CHUNK', OTHER[1])


def _handle():
    rowptr = torch.tensor([0, 70, 70, 200, 203], dtype=torch.int64)
    return rowptr, torch.zeros(203, dtype=torch.int64)


def _plan():
    """rows 0 (70 slots: 2 chunks of 48) and 2 (130: 3) of :func:`_handle` at (64, 48)"""
    return _native.HubPlan(torch.tensor([0, 2]), torch.tensor([0, 2, 5]), 2, 5, *OWN)


def test_fields_in_order():
    assert _native.HubPlan._fields == ('rows', 'chunk_ptr', 'n_hub', 'n_chunks', 'threshold',
                                       'chunk')
    plan = _plan()
    assert plan[0] is plan.rows and plan[1] is plan.chunk_ptr and plan[2] == plan.n_hub == 2
    assert tuple(_native.no_hubs(*OWN)) == (None, None, 0, 0, 64, 48)


def test_csr_takes_the_pair_from_the_plan(other_module_pair):
    rowptr, col = _handle()
    plan = _plan()
    g = _native._csr(rowptr, col, 4, plan)
    assert (g.hub_threshold, g.hub_chunk) == OWN
    assert (g.n_hub, g.n_chunks) == (2, 5)
    assert g.hub_rows == plan.rows.data_ptr() and g.hub_chunk_ptr == plan.chunk_ptr.data_ptr()
    assert g.rowptr == rowptr.data_ptr() and g.col == col.data_ptr() and g.n_rows == 4


def test_spmm_args_take_the_pair_from_the_plan(other_module_pair):
    plan = _plan()
    a = SpmmArgs()
    _native._hub_args(a, plan)
    assert (a.hub_threshold, a.hub_chunk) == OWN
    assert (a.n_hub, a.n_chunks) == (2, 5)
    assert a.hub_rows == plan.rows.data_ptr() and a.hub_chunk_ptr == plan.chunk_ptr.data_ptr()
    # ... and the six loose arguments of the compiled routes are the plan itself
    assert tuple(_native._hub6(plan)) == (plan.rows, plan.chunk_ptr, 2, 5, *OWN)


@pytest.mark.parametrize('hub', [None, _native.no_hubs(*OWN)], ids=['None', 'no-hub plan'])
def test_no_hub_rows(other_module_pair, hub):
    rowptr, col = _handle()
    g = _native._csr(rowptr, col, 4, hub)
    assert g.n_hub == 0 and g.n_chunks == 0 and g.hub_rows is None and g.hub_chunk_ptr is None
    # (no kernel reads the pair without hub rows; None fills the module's, a plan its own)
    assert (g.hub_threshold, g.hub_chunk) == (OTHER if hub is None else OWN)
    a = SpmmArgs()
    _native._hub_args(a, hub)
    assert a.n_hub == 0 and a.n_chunks == 0 and a.hub_rows is None and a.hub_chunk_ptr is None
    assert (a.hub_threshold, a.hub_chunk) == (0, 0)       # left at zero, as the struct was made
    six = _native._hub6(hub)
    assert tuple(six[:4]) == (None, None, 0, 0) and tuple(six[4:]) == (OTHER if hub is None else OWN)


def test_csr_keeps_its_tensors_alive():
    rowptr, col = _handle()
    plan = _plan()
    refs = [weakref.ref(t) for t in (rowptr, col, plan.rows, plan.chunk_ptr)]
    g = _native._csr(rowptr, col, 4, plan)
    del rowptr, col, plan
    gc.collect()
    assert all(r() is not None for r in refs)
    assert g.rowptr == refs[0]().data_ptr()
    del g
    gc.collect()
    assert all(r() is None for r in refs)


def test_plan_of_no_rows_records_what_it_was_asked_for(monkeypatch, other_module_pair):
    """the early return of ``hub_plan``: before the library is loaded"""
    from pytorch_geometric_amd import _lib

    def no_library():
        raise AssertionError('hub_plan of no rows loaded the library')

    monkeypatch.setattr(_lib, 'load', no_library)
    monkeypatch.setattr(_native, '_require_device', lambda *t: None)    # (CPU tensors here)
    for rowptr in (torch.zeros(1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)):
        assert tuple(_native.hub_plan(rowptr, *OWN)) == (None, None, 0, 0, *OWN)
        # the defaults are read from the module when the plan is made
        assert tuple(_native.hub_plan(rowptr)) == (None, None, 0, 0, *OTHER)
        assert tuple(_native.hub_plan(rowptr, chunk=7)) == (None, None, 0, 0, OTHER[0], 7)
