"""CPU-only checks of how the library is cut into translation units (csrc/mw_dycore_int.h has the unit map).

Without relocatable device code every unit is a code object of its own inside the .so: a kernel template instantiated from two units, or a
non-template kernel in a header that two units include, would be emitted into both.  Every kernel must sit in the library exactly once."""
import collections
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "miniweatherml_amd", "csrc")


def test_no_kernel_sits_in_two_code_objects(mw):
    """The `.kd` kernel descriptor names of the embedded gfx950 code objects (the regular expression of conftest._compiled_dycore_kernels,
    every family): no name occurs more often than the rarest one does."""
    from miniweatherml_amd import capi
    blob = open(capi.LIB_PATH, "rb").read()
    count = collections.Counter(m.group(1).decode() for m in re.finditer(rb"(_ZN2mw(\d+)([0-9A-Za-z_]+))\.kd\x00", blob))
    assert len(count) > 200, len(count)                               # (the dispatcher's instantiations alone are more)
    least = min(count.values())
    assert {n: c for n, c in count.items() if c > least} == {}


def test_every_source_of_csrc_is_built(mw):
    from miniweatherml_amd import build
    assert sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp"))) == sorted(build.SOURCES)
