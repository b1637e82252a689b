"""The table of tests/pipeline_order_cases.py against include/slam_hip.h and against the legs that exist: every device
entry point has a leg of tests/test_gpu_pipeline_order.py or a stated exemption, every leg of the table is written, and
nothing is written that the table does not know."""
import os
import re

import pipeline_order_cases as C
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "slam_hip.h")
GPU_FILE = os.path.join(ROOT, "tests", "test_gpu_pipeline_order.py")


def declared():
    with open(HEADER) as f:
        return C.dev_entry_points(f.read())


def test_the_header_is_parsed():
    names = declared()
    assert len(names) >= 37 and "slam_replay_dev" in names and "slam_grid_view_gain_dev" in names
    assert all(n.startswith("slam_") and n.endswith("_dev") for n in names)


def test_every_device_entry_point_is_a_leg_or_exempt():
    legs = {entry for entry, _ in C.LEGS.values()}
    exempt = {name.split("[")[0] for name in C.EXEMPT}
    missing = [n for n in declared() if n not in legs and n not in exempt]
    assert not missing, "no leg and no exemption for %s: decide how a call to it is ordered behind a pipelined replay" % missing


def test_exemptions_are_few_named_and_reasoned():
    names = declared()
    with open(HEADER) as f:
        header = f.read()
    for name, reason in C.EXEMPT.items():
        base = name.split("[")[0]
        assert base in names or re.search(r"\b%s\s*\(" % base, header), name       # a real entry point
        assert len(reason.split()) >= 4, name
    # the pipeline's own stages are exempt because a join would undo the overlap; they must stay the only ones without one
    for stage in ("slam_replay_dev[piped]", "slam_grid_reset", "slam_grid_finalize_dev"):
        assert stage in C.EXEMPT
    assert len(C.EXEMPT) <= len(C.LEGS) // 2
    # slam_replay_dev is both: exempt when piped, a leg when it follows a piped replay
    both = {n.split("[")[0] for n in C.EXEMPT} & {e for e, _ in C.LEGS.values()}
    assert both == {"slam_replay_dev"}


def test_every_leg_names_a_declared_function_and_a_kind():
    with open(HEADER) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for leg, (entry, kind) in C.LEGS.items():
        assert re.search(r"\b%s\s*\(" % entry, header), (leg, entry)
        assert kind in ("grid", "M", "P-in", "P-out", "stream"), leg
        assert re.fullmatch(r"[a-z0-9_]+", leg)


def test_the_gpu_file_has_exactly_the_legs_of_the_table():
    with open(GPU_FILE) as f:
        written = re.findall(r"^def leg_([a-z0-9_]+)\(", f.read(), flags=re.M)
    assert len(written) == len(set(written))
    assert sorted(written) == sorted(C.LEGS)

