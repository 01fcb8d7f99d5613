"""Which path each solver configuration takes, pinned as a whole (tools/record_path_ledger.py).

Every row of the recorder's tables runs one solve of fixed length under the per-kernel event
profile; its record -- launch count and byte total of every profile class, ``band``, ``orth``,
``inner_iters``, ``restarts``, ``info`` -- must equal the committed one
(tests/golden/path_ledger.json) exactly.  The byte totals are host-computed doubles, summed in
launch order: ``==``.  The other GPU tests spot-check single classes; a host-driver change that
sends a configuration down another path, drops a launch or alters a byte model fails here.
A deliberate change re-records the fixture with the tool.

Independent of the fixture, the rows that name a ``band`` expectation are held to it: a lagged
preconditioner (values updated, no refresh) must leave the band step.
"""
import functools
import json
import os
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_path_ledger as ledger  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "path_ledger.json")) as f:
        return json.load(f)


def _same(got, want, tag):
    got = json.loads(json.dumps(got))   # tuples -> lists, as the fixture was written
    for k in sorted(set(got) | set(want)):
        if k != "classes":
            assert got.get(k) == want.get(k), (tag, k, got.get(k), want.get(k))
    gc, wc = got["classes"], want["classes"]
    assert sorted(gc) == sorted(wc), (tag, sorted(set(gc) ^ set(wc)))
    for cls in wc:
        assert gc[cls] == wc[cls], (tag, cls, gc[cls], wc[cls])


def test_tables_match_fixture():
    g = _golden()
    assert sorted(g["rows"]) == sorted(r["id"] for r in ledger.ROWS)
    assert sorted(g["ranks"]) == sorted(ledger.RANK_GROUPS)
    for group, (world, rows) in ledger.RANK_GROUPS.items():
        assert sorted(g["ranks"][group]) == sorted(r["id"] for r in rows)
        assert all(len(v) == world for v in g["ranks"][group].values())


@pytest.mark.parametrize("row", ledger.ROWS, ids=[r["id"] for r in ledger.ROWS])
def test_row(vk_lib, gpu, row):
    rec, _ = ledger.run_row(vk_lib, gpu, row)
    print(row["id"], json.dumps(rec))
    if row["band"] is not None:
        assert rec["band"] == row["band"], (row["id"], rec["band"])
    _same(rec, _golden()["rows"][row["id"]], row["id"])


@pytest.mark.parametrize("group", list(ledger.RANK_GROUPS))
def test_ranks(vk_lib, group):
    """Host-staged communicator, the ranks share the GPU: every rank's record."""
    world, rows = ledger.RANK_GROUPS[group]
    got = ledger.run_group(group)
    for row in rows:
        for r in range(world):
            rec = got[row["id"]][r][0]
            print(group, row["id"], r, json.dumps(rec))
            if row["band"] is not None:
                assert rec["band"] == row["band"], (group, row["id"], r, rec["band"])
            _same(rec, _golden()["ranks"][group][row["id"]][r], (group, row["id"], r))
