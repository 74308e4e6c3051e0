"""av1mi_encode_file's hand-over between its reader, its encode threads and its writer (av1-base_amd/csrc/av1mi_pipeline.h) run without a
GPU over a fake item whose work sleeps - longer for earlier items, so that later items finish first (tests/host/pipeline_host.cpp) -
plain, under AddressSanitizer + UndefinedBehaviorSanitizer (the leak check is the witness that every item is destroyed) and under
ThreadSanitizer.  Each build's program runs once, over all the cases, under a time limit: the sleeps of a case add up to under 50 ms and
those of all cases to under a second, so 60 s is a guard against a deadlock, not a measurement, and running into it is a failure."""
import os
import shutil

import pytest

import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "host", "pipeline_host.cpp")]
ITEMS = 40
BUILDS = {"plain": False, "asan_ubsan": True, "tsan": host_build.THREAD_SANITIZE}
# (workers, items, failing item or -1): every worker count clean and with no item at all; the first, a middle and the last item failing
RUNS = [(w, ITEMS, -1) for w in (1, 2, 4)] + [(w, 0, -1) for w in (1, 4)] + [(w, ITEMS, k) for w in (1, 2, 4) for k in (0, ITEMS // 2, ITEMS - 1)]


@pytest.fixture(scope="module", params=list(BUILDS))
def program(request, tmp_path_factory):
    """the program under one of the builds, and every run's fields: by g++ where there is one (the header is plain C++), or by the other
    host compiler where that one's sanitizer runtime works and g++'s does not"""
    d = tmp_path_factory.mktemp("pipeline_" + request.param)
    flags = host_build.SANITIZE if BUILDS[request.param] is True else BUILDS[request.param]
    cxxs = [c for c in (shutil.which("g++"), host_build.host_cxx(gcc=True)) if c]
    cxx = next((c for c in cxxs if not flags or host_build.sanitizers_work(c, d, flags)), cxxs[0])
    out = host_build.run_program(cxx, SOURCES, d / "pipeline_host", args=[a for run in RUNS for a in run], sanitized=BUILDS[request.param],
                                 extra=["-pthread"], timeout=60)
    assert out.returncode == 0, "%s: %s" % (request.param, out.stdout[-500:] + out.stderr[-3000:])
    lines = out.stdout.splitlines()
    assert len(lines) == len(RUNS)
    return {run: dict(t.split("=", 1) for t in line.split()) for run, line in zip(RUNS, lines)}


def _ids(row):
    return [int(x) for x in row["written"].split(",") if x]


def test_items_are_written_in_order_on_the_submitting_thread(program):
    for workers in (1, 2, 4):
        r = program[(workers, ITEMS, -1)]
        assert _ids(r) == list(range(ITEMS)) and r["err"] == "0" and r["submitted"] == r["seen"] == str(ITEMS)
        assert r["wrong_thread"] == "0" and r["unworked"] == "0" and r["bad_worker"] == "0"


def test_outstanding_items_stay_within_twice_the_workers(program):
    for (workers, items, _), r in program.items():
        assert int(r["max_outstanding"]) <= 2 * workers, (workers, r)
        assert items == 0 or int(r["max_outstanding"]) >= 1


def test_every_item_is_destroyed_once(program):
    for run, r in program.items():
        assert r["made"] == r["gone"] == r["submitted"] == r["seen"], run


def test_no_items_at_all(program):
    for workers in (1, 4):
        r = program[(workers, 0, -1)]
        assert (r["submitted"], r["seen"], r["written"], r["err"]) == ("0", "0", "", "0")


def test_first_failure_stops_the_writing_and_every_item_is_still_seen(program):
    """the caller-side rule of av1mi_file.cpp: items 0 .. k-1 are written, k's code is reported, and what was submitted behind k still
    passes through the writer (to be freed and counted)"""
    for workers in (1, 2, 4):
        for k in (0, ITEMS // 2, ITEMS - 1):
            r = program[(workers, ITEMS, k)]
            assert _ids(r) == list(range(k)) and r["err"] == str(100 + k), (workers, k)
            assert k + 1 <= int(r["submitted"]) <= min(ITEMS, k + 1 + 2 * workers), (workers, k)
