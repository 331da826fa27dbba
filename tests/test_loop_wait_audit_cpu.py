"""tools/loop_wait_audit.py on the x/z marching unit: no k_xz_state instantiation of the landed() design waits for the loads of a level
right behind them.  (vmcnt retires in order and counts stores: a value that the compiler consumes where it is declared puts a vmcnt(0) at the
top of the iteration, behind the loads just issued and the previous level's stores -- k_xz_state<3, .., MODE 1, VAP> did, for the row-map word
of its lean predicate, and paid a memory round trip per level.)

The tool's two thresholds are the conditions: a wait fewer than 32 instructions behind a load it waits for, with at least 8 loads of the
iteration outstanding.  The loops of the design sit at several hundred instructions; the faulty one sat at 1.

Two families of k_xz_state are not of that design and the tool does flag them, 30-31 instructions behind the load: the neighbour-load form
for nens > 1 (N1 = false), which fetches the x neighbours of a level from memory in mid-iteration and needs them for the reconstruction
right away, and the member-co-located form (MT).  They are listed in profiles/r08_loop_wait_audit.txt; here those five instantiations may be flagged, at the
distance they keep today, and no other instantiation may.

No GPU needed: hipcc compiles the unit to device assembly."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc is not installed")


# the instantiations that are not of the design (see above) and are flagged as they stand: by name, and with the distance their waits keep,
# so that neither a new form of those families nor one of these at 1-2 instructions behind its loads goes through
KNOWN = {
    "k_xz_state<1, false, 0, 0, 0, 5, false, false>": 30,
    "k_xz_state<2, false, 0, 0, 0, 5, false, false>": 30,
    "k_xz_state<3, false, 0, 0, 0, 5, false, false>": 30,
    "k_xz_state<3, false, 1, 0, 0, 5, false, false>": 30,
    "k_xz_state<3, true, 1, 1, 1, 3, true, false>": 30,
}


@pytest.fixture(scope="module")
def rows():
    import loop_wait_audit
    assert (loop_wait_audit.NEAR, loop_wait_audit.MIN_LOADS) == (32, 8)
    return [r for r in loop_wait_audit.audit_unit("mw_march_xz.hip") if r["kernel"].startswith("k_xz_state<")]


def test_no_marching_loop_of_the_design_waits_behind_its_loads(rows):
    assert not any(r["truncated"] for r in rows)
    flagged = sorted({r["kernel"] for r in rows if r["findings"]})
    print("flagged:", flagged)
    assert set(flagged) <= set(KNOWN), sorted(set(flagged) - set(KNOWN))
    for r in rows:
        for f in r["findings"]:
            assert f["behind_load"] >= KNOWN[r["kernel"]], (r["kernel"], f)


def test_the_vapour_forms_wait_in_front_of_their_stores(rows):
    """the four instantiations of the headline path: every load of the marching loop meets its first wait several hundred instructions on --
    but for the refetch of the lean bits (chunks of more than 64 levels), a single load with nothing else of the iteration in flight"""
    for stage, mode in ((1, 0), (2, 0), (3, 0), (3, 1)):
        name = "k_xz_state<%d, true, %d, 1, 1, 5, false, true>" % (stage, mode)
        mine = [r for r in rows if r["kernel"] == name]
        assert mine, name
        for r in mine:
            assert not r["findings"], (name, r["findings"])
            far = [d for d, _ in r["load_to_wait"] if d >= 32]
            assert len(far) >= 8 and min(far) >= 185, (name, r["load_to_wait"])
