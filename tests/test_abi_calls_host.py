"""The Python layer hands the C ABI what it handed it before it was rebuilt around one call record: entry names, scalars,
null / non-null pointers and the contents of coords, channels, radii, offsets, mvx_xform records and packed poses, bit for bit,
for the host-array entries (tests/abi_calls.py). The expectation, tests/golden/abi_calls_host.json, was written by
tools/record_abi_calls.py on the parent of that change, never by the code under test. No GPU."""
import json
import os

import pytest

from tests import abi_calls


@pytest.fixture(scope="module")
def recorded():
    return abi_calls.record()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "abi_calls_host.json")) as f:
        return json.load(f)


def test_the_table_is_the_recorded_one(recorded, golden):
    assert sorted(recorded["rows"]) == sorted(golden["rows"]) and len(golden["rows"]) == len(abi_calls.table())


@pytest.mark.parametrize("rid", [row[0] for row in abi_calls.table()])
def test_the_library_sees_the_same_call(rid, recorded, golden):
    got = json.loads(json.dumps(recorded["rows"][rid]))  # (tuples to lists, as the file holds them)
    assert got == golden["rows"][rid]  # (an array's name holds its dtype, length and digest ...)


def test_the_arrays_are_the_recorded_ones(recorded, golden):
    assert recorded["arrays"] == golden["arrays"]  # (... and these are the bytes behind the names)


def test_the_table_covers_what_it_should(golden):
    arrays, golden = golden["arrays"], golden["rows"]
    used = {v for row in golden.values() for c in row["calls"] for k, v in c.items() if k.endswith("@") and isinstance(v, str)}
    used |= {v for row in golden.values() for c in row["calls"] for rec in c.get("xforms@", []) for v in rec.values() if isinstance(v, str)}
    assert used == set(arrays)
    entries = {c["entry"] for row in golden.values() for c in row["calls"]}
    assert entries == {"mvx_forward_features", "mvx_forward_types", "mvx_forward_single", "mvx_forward_features_batch",
                       "mvx_forward_types_batch", "mvx_forward_single_batch", "mvx_forward_views"}
    assert all(len(row["calls"]) == 1 for row in golden.values())
    padded = [golden[r]["calls"][0] for r in ("forward_types-padded", "forward_batch-padded", "forward_views-padded")]
    assert all(c["C"] == abi_calls.CH and c["radii@"].startswith(f"float32x{abi_calls.CH}:") for c in padded)  # three radii given, one padded on
    posed = golden["forward_posed_batch-features-scalar-centers"]["calls"][0]["xforms@"]
    assert len(posed) == abi_calls.B and all("pose" in rec for rec in posed)
