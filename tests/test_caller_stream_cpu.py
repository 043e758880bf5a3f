"""CPU guard of the caller-stream suite: every prototype of include/gelato_amd.h that takes a `void* stream` has a case in
tests/stream_cases.py (run on the GPU by tests/test_caller_stream.py).  An entry point added later without one fails here, on any
machine."""
import os
import re

from conftest import ROOT
import stream_cases as SC


def stream_entry_points():
    """names of the header's functions with a `void* stream` parameter"""
    text = open(os.path.join(ROOT, "include", "gelato_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)          # comments name parameters too
    found = set()
    for m in re.finditer(r"\bint\s+(gel_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            found.add(m.group(1))
    return found


def test_every_stream_entry_point_has_a_caller_stream_case():
    names = stream_entry_points()
    assert len(names) >= 16 and "gel_sync" in names and "gel_eval_batch_device" in names      # the parser sees the header
    assert names == set(SC.CASES), (sorted(names - set(SC.CASES)), sorted(set(SC.CASES) - names))
    assert all(len(v) > 0 for v in SC.CASES.values())


def test_case_ids_are_unique_per_case():
    ids = {}
    for lst in SC.CASES.values():
        for cid, make in lst:
            assert ids.setdefault(cid, make) is make, cid
    assert len(SC.all_cases()) == len(ids)
