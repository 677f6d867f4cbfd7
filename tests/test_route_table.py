"""The decoding route of every kind of generate() call, replayed on the CPU against tests/golden/route_table.json.gz.

The table was recorded by tools/route_table.py at the commit before eilev_amd/route.py existed: the same grid, driven through the same
real generate() / beam_decode / t5_beam / sample_decode / t5_sample, must end in the same leaves with the same arguments, records and
refusals now that eilev_amd/route.py plan_decode is the one place that chooses.
"""
import importlib.util
import os

import pytest

from eilev_amd import route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_ROUTES = ("beam_device", "sample_host", "search_host")


@pytest.fixture(scope="module")
def replay():
    """(tool, points, table, plans): the grid replayed once on the working tree; plans[i] — every Plan made while point i ran."""
    spec = importlib.util.spec_from_file_location("route_table", os.path.join(ROOT, "tools", "route_table.py"))
    rt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rt)
    real, made, plans = route.plan_decode, [], []

    def spy(*a, **k):
        made.append(real(*a, **k))
        return made[-1]

    def observe(p, entry):
        plans.append(list(made))
        made.clear()

    route.plan_decode = spy
    try:
        points = rt.grid()
        table = rt.build_table(points, observe)
    finally:
        route.plan_decode = real
    return rt, points, table, plans


def test_the_table_is_the_recorded_one(replay):
    rt, points, table, _ = replay
    want = rt.load_table(os.path.join(ROOT, "tests", "golden", "route_table.json.gz"))
    assert want["keys_sha256"] == table["keys_sha256"], "the grid is not the recorded one"
    assert len(want["points"]) == len(points)
    for p, i, j in zip(points, table["points"], want["points"]):
        assert table["outcomes"][i] == want["outcomes"][j], rt.key_of(p)
    rt.assert_covers(points, table)  # every leaf, route, refusal, fp8 cause and host condition is in it, for both language models


def test_the_plan_names_the_route_that_ran(replay):
    rt, points, table, plans = replay
    seen = {"opt": set(), "t5": set()}
    for p, i, made in zip(points, table["points"], plans):
        ran = rt.route_of(table["outcomes"][i])
        for plan in made:
            assert bool(plan.host_reasons) == (plan.route in HOST_ROUTES), (rt.key_of(p), plan)
            assert ran is None or plan.route == ran, (rt.key_of(p), plan.route, ran)
            seen[p["lm"]].update(plan.host_reasons)
        assert made or ran is None, rt.key_of(p)  # no leaf is reached without a plan
    assert seen["opt"] >= set(rt.HOST_REASONS) and seen["t5"] >= set(rt.HOST_REASONS) - {"trace"}


def test_fp8_is_refused_before_the_encode_exactly_off_the_captured_routes(replay):
    """generate(kv_cache_dtype="fp8") on OPT raises before _encode exactly when the bf16 call of the same arguments does not reach one of
    the three captured routes (beside it: a head size other than 80 / 128, context=, prompt lookup, which are refused where bf16 runs)."""
    rt, points, table, _ = replay
    entry = {rt.key_of(p): table["outcomes"][i] for p, i in zip(points, table["points"])}
    causes, checked = set(), 0
    for p in points:
        if p["entry"] != "generate" or p["kv"] != "fp8":
            continue
        e = entry[rt.key_of(p)]
        refused = bool(rt.fp8_causes(e))
        causes.update(rt.fp8_causes(e))
        if refused:
            assert e["encodes"] == 0 and not e["calls"], rt.key_of(p)
        if p["lm"] == "t5" or p["extra"] in ("context", "lookup") or p["off"] == "head_size":
            assert "raises" in e and e["encodes"] == 0, rt.key_of(p)  # (flan-t5 with context= is refused as a context call first)
            continue
        twin = entry[rt.key_of(dict(p, kv="bf16"))]
        captured = rt.route_of(twin) in route.CAPTURED
        assert refused == (not captured), rt.key_of(p)
        if captured:  # served: one encode, the twin's leaf, the fp8 cache asked of it
            assert e["encodes"] == 1 and [c[0] for c in e["calls"]] == [c[0] for c in twin["calls"]], rt.key_of(p)
            assert all(c[1]["kv_dtype"] == "fp8" for c in e["calls"]), rt.key_of(p)
        checked += 1
    assert checked >= 1920 and causes == set(rt.FP8_CAUSES)  # (1920: OPT's generate() fp8 points of the all-on product)
