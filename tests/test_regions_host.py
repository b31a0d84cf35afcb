"""CPU-only: the page-regions entry point's limits and argument checks (every call returns before a launch: the pointers are dummies),
the default class -> kind table, and the refusal of host tensors."""
import numpy as np
import pytest
import torch

from gnn_tableextraction_amd import _lib, graph as G
from gnn_tableextraction_amd.components.graphs import postprocessing as PP

_P = 0x10000          # a dummy 16-byte aligned address: never dereferenced, no call below reaches a launch


def _call(lib, **change):
    args = dict(indptr=_P, indices=_P, node_off=_P, n_pages=3, n_nodes=100, max_page_nodes=50, group=_P, bbox=_P, comp=_P,
                region_box=_P, region_count=_P, stream=None)
    assert set(change) <= set(args)
    args.update(change)
    return lib.gte_page_regions(*[args[k] for k in ("indptr indices node_off n_pages n_nodes max_page_nodes group bbox comp "
                                                    "region_box region_count stream").split()])


def test_every_page_the_graph_builder_accepts_is_accepted():
    lib = _lib.load()
    assert lib.gte_region_max_page_nodes() >= lib.gte_knn_max_page_nodes() > 0


def test_bad_arguments_return_error_codes_without_launching():
    lib = _lib.load()
    limit = lib.gte_region_max_page_nodes()
    assert _call(lib, max_page_nodes=limit + 1) == -4 and b"exceeds" in lib.gte_last_error()       # GTE_ERR_UNSUPPORTED
    assert _call(lib, n_pages=-1) == -1                                                           # GTE_ERR_INVALID_ARGUMENT
    assert _call(lib, n_nodes=-1) == -1 and _call(lib, max_page_nodes=-1) == -1
    assert _call(lib, n_pages=0) == -1                    # nodes without a page
    for name in ("comp", "region_box", "region_count", "indptr", "indices", "node_off", "group", "bbox"):
        assert _call(lib, **{name: None}) == -1 and b"null" in lib.gte_last_error(), name
    assert _call(lib, bbox=_P + 4) == -1 and b"aligned" in lib.gte_last_error()
    assert _call(lib, region_box=_P + 8) == -1
    assert _call(lib, n_nodes=-1, max_page_nodes=limit + 1) == -1      # wrong in two ways: the check that stands first
    assert _call(lib, max_page_nodes=limit + 1, comp=None) == -4
    assert _call(lib, n_nodes=0, n_pages=0, comp=None) == 0            # nothing to do
    with pytest.raises(_lib.GteError):
        _lib.check(_call(lib, n_pages=-1), "probe")


def test_default_class_group_merges_the_table_classes_and_drops_other():
    from gnn_tableextraction_amd.components.graphs.loader import ORIGIN_TO_CONV
    table = PP.DEFAULT_CLASS_GROUP
    assert len(table) == 9 and table[0] == -1
    conv_to_origin = {v: k for k, v in ORIGIN_TO_CONV.items() if v is not None}
    for conv, kind in enumerate(table):
        origin = conv_to_origin[conv]
        if origin in (7, 8, 10):                          # column header, spanning cell, table cell -> TABLE
            assert kind == 4
        elif origin == 0:
            assert kind < 0
        else:
            assert kind == origin                         # text 1, title 2, list 3, figure 5, caption 6
    assert {PP.GROUP_NAMES[k] for k in table if k >= 0} == {"text", "title", "list", "table", "figure", "caption"}


def test_page_regions_refuses_host_tensors():
    g = G.PageGraph([0, 1], [1, 0], 2)
    with pytest.raises(_lib.GteError):
        PP.page_regions(g, torch.zeros(2, dtype=torch.int32), torch.zeros((2, 4), dtype=torch.int32))
