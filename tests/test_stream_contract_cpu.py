"""The record table of tests/stream_contract_cases.py against include/rwh.h, without a GPU: every RWH_API function that takes a
stream has a record or a stated exemption; the exemptions are the entry points
whose header comment says that they synchronise; and every record's reference can be made on the host and tells its inputs apart."""
import os
import re

import numpy as np
import pytest

import sequence_cases as sc
import stream_contract_cases as scc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rwh.h")


def _declarations():
    """name -> (parameter list, the comment in front of the declaration's group) for every RWH_API function of the header."""
    text = open(HEADER).read()
    out = {}
    for m in re.finditer(r"^RWH_API\s+[\w\s\*]+?\b(rwh_\w+)\s*\(([^;]*?)\)\s*;", text, re.M | re.S):
        end = text.rfind("*/", 0, m.start())
        begin = text.rfind("/*", 0, end)
        out[m.group(1)] = (" ".join(m.group(2).split()), text[begin:end])
    return out


def test_every_entry_point_with_a_stream_has_a_record_or_a_reason():
    decl = _declarations()
    assert len(decl) > 100 and "rwh_stitch_sequence_labels_maps_proj" in decl
    streamed = {name for name, (params, _) in decl.items() if re.search(r"void\s*\*\s*stream\b", params)}
    assert "rwh_host_refit" not in streamed and "rwh_warp_plan" not in streamed and len(streamed) > 40
    recorded = {r.entry for r in scc.RECORDS.values()}
    groups = [recorded, set(scc.EXEMPT), set(scc.EXEMPT_LAB)]
    for i, a in enumerate(groups):
        for b in groups[i + 1:]:
            assert not a & b, sorted(a & b)
    missing, unknown = streamed - set().union(*groups), set().union(*groups) - streamed
    assert not missing, "no record and no stated exemption: %s" % sorted(missing)
    assert not unknown, "not an entry point with a stream: %s" % sorted(unknown)
    assert all(isinstance(v, str) and v for d in (scc.EXEMPT, scc.EXEMPT_LAB) for v in d.values())


def test_the_exemptions_are_what_the_header_says_synchronises():
    decl = _declarations()
    assert set(scc.EXEMPT) == {"rwh_sequence_seams", "rwh_sequence_seams_proj", "rwh_ransac_run"}
    assert set(scc.EXEMPT_LAB) == {"rwh_lab_clock_probe"}
    for name in scc.EXEMPT:
        assert "synchronis" in decl[name][1].lower(), name
    assert "lab" in decl["rwh_lab_clock_probe"][1].lower()
    head = open(HEADER).read().split("*/")[0]
    assert "except where an entry" in head and "rwh_ransac_run" in head and "rwh_sequence_seams*" in head


@pytest.fixture(scope="module")
def lib():
    return sc.library()


@pytest.mark.parametrize("name", list(scc.RECORDS))
def test_a_records_reference_tells_its_inputs_apart(lib, name):
    """On the host: the record is made, refresh gives three different sets of inputs, and a record with a host reference expects
    three different results for them (a record without a bit-exact reference is compared with an eager call, on the GPU)."""
    live = scc.RECORDS[name].make(lib)
    snaps = [live.refresh(seed) for seed in (0, 1, 2)]
    differ = lambda a, b: any(not np.array_equal(x, y) for x, y in zip(a, b))
    if live.constant:
        assert not live.inputs                     # no device input to refresh: the call's result is a function of its host arguments
        return
    assert differ(snaps[0], snaps[1]) and differ(snaps[0], snaps[2]) and differ(snaps[1], snaps[2])
    assert live.host_args is not None and all(isinstance(a, np.ndarray) for a in live.host_args)
    if live.shadow is None:
        wants = [live.expected(s) for s in snaps]
        assert [w.size for w in wants[0]] == [o.nbytes for o in live.outputs]
        assert differ(wants[0], wants[1]) and differ(wants[0], wants[2]) and differ(wants[1], wants[2])
