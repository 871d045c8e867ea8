"""The GEMM dispatch answers, for every descriptor of the route sweep (tests/gemm_route_cases.py), what the library answered before the
dispatch became one route (tests/golden/gemm_route_table.json): which kernel each launch runs, how many launches, the family, the split-K
slices, the statistics slabs and the three capability queries; and it rejects what it rejected, with the same message.  Host only: without a
device cu_count() is the MI355X's 256 CUs, which is what the table was recorded with."""
import json

import pytest
import torch

import gemm_route_cases as RC
import kernel_form_cases as KC
from sduss_amd import lib as L


# Messages of the recorded table that changed because two statements of one rule -- one for the descriptor's own problem, one for a problem of
# a grouped launch -- became one (validate_problem, gemm_dispatch.cpp): the grouped wording went.
_G = "gemm: grouped launch: "
MERGED = {
    _G + "rows_per_batch required": "gemm: rows_per_batch required",
    _G + "bad input row remap": "gemm: bad input row remap",
    _G + "bad output row remap": "gemm: bad output row remap",
    _G + "operand exceeds 32-bit indexing": "gemm: operand exceeds 32-bit indexing",
    _G + "QKV needs whole batches and ldvt >= MX_VT_LD(keys per batch)": "gemm: QKV needs M % rows_per_batch == 0",
    "conv3x3: grouped launch: a problem's output grid does not match its input grid / stride / rows":
        "conv3x3: output grid does not match input grid / stride",
}


@pytest.fixture(scope="module")
def table():
    with open(RC.TABLE) as f:
        return json.load(f)


def test_sweep_reaches_every_answer(table):
    """conditions on the sweep itself, checked on the recorded answers"""
    rows = [table["answers"][i] for v in table["rows"].values() for i in v]
    assert len(rows) >= 3000
    named = {table["names"][k] for r in rows if r[0] != -1 for k in r[0]}
    assert named | KC.NOT_COVERED == set(table["names"]) == set(L.gemm_kernel_names())
    assert {r[2] for r in rows} == set(range(7))                 # every MX_FORM_* value (mxdenoise.h: 0 .. 6)
    assert {r[3] for r in rows} == {1, 2, 3, 4}                  # split-K slices
    assert {r[1] for r in rows} == {1, 2}                        # launches
    for col in (5, 6, 7):                                        # ln_prefers_pass, gn_partials_supported, ln_final_supported
        assert {r[col] for r in rows} == {0, 1}
    assert 0 in {r[4] for r in rows} and max(r[4] for r in rows) > 0
    assert any(r[0] == -1 for r in rows)                         # descriptors no instantiation serves


def test_routes_match_the_recorded_table(table):
    names = L.gemm_kernel_names()
    assert names == table["names"]
    cases = RC.route_cases()
    count = {}
    wrong = []
    for c in cases:                                              # the table lists a variant's rows in the generator's order
        v = RC.variant_of(c["name"])
        i = count[v] = count.get(v, -1) + 1
        got = RC.answers_of(RC.desc_of(c), c["kind"] == "conv", names)
        want = table["answers"][table["rows"][v][i]]
        if got != want:
            wrong.append((c["name"], got, want))
    assert {v: n + 1 for v, n in count.items()} == {v: len(r) for v, r in table["rows"].items()}
    assert not wrong, f"{len(wrong)} of {len(cases)} descriptors answer differently, first: {wrong[:5]}"


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls mx_gemm with fake pointers: a wrongly accepted descriptor must never reach a GPU")
def test_rejections_match_the_recorded_table(table):
    lib = L.load()
    want = dict(table["rejections"])
    assert [lib.mx_gemm(None, None), lib.mx_last_error().decode()] == want.pop("null_descriptor")
    cases = RC.rejection_cases()
    assert [name for name, _, _ in cases] == list(want)
    for name, case, mut in cases:
        status, msg = RC.rejection_of(name, case, mut)
        assert status != 0 and want[name][0] != 0, name
        assert msg == MERGED.get(want[name][1], want[name][1]), name


