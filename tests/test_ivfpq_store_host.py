"""No GPU: the IVF-PQ store factory validates its arguments on the host, and the selected-view entry point is in the
signature table, the header and the built library."""
import re
from pathlib import Path

import pytest

from eioku_amd import _lib, ivfpq

ROOT = Path(__file__).resolve().parent.parent


def test_store_index_factory_validates_on_the_host():
    build = ivfpq.store_index_factory(nlist=16, m=8, nprobe=4)
    assert callable(build)
    for bad in (dict(nlist=0, m=8, nprobe=1), dict(nlist=16, m=0, nprobe=1), dict(nlist=16, m=8, nprobe=0),
                dict(nlist=16, m=8, nprobe=17), dict(nlist=16.5, m=8, nprobe=1), dict(nlist=16, m="8", nprobe=1)):
        with pytest.raises(ValueError):
            ivfpq.store_index_factory(**bad)
    with pytest.raises(ValueError, match="d/m"):
        build(65)   # not a multiple of m
    with pytest.raises(ValueError, match="d/m"):
        build(256)  # 32-dim sub-vectors


def test_search_many_names_its_limit_without_a_gpu():
    ix = ivfpq.IndexIVFPQ.__new__(ivfpq.IndexIVFPQ)  # the check comes before anything touches the device
    with pytest.raises(ValueError, match=r"k <= 32"):
        ix.search_many(None, 33)


def test_select_view_is_in_the_table_the_header_and_the_library(built_lib):
    name = "eioku_ivfpq_select_view"
    restype, argtypes = _lib.SIGNATURES[name]
    header = (ROOT / "include" / "eioku_hip.h").read_text()
    proto = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert proto, "not declared in include/eioku_hip.h"
    assert len([a for a in proto.group(1).split(",") if a.strip()]) == len(argtypes) == 20
    assert hasattr(built_lib, name)
