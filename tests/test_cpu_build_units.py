"""tools/build_rev_lib.py's unit list for OTHER revisions' sources: round-4 sources (22c4d2a)
define every fused entry once per (mode, finalisation) source and the 16-bit entries once, so splitting them into
FEDAVG_EPI_PART=1/2 and FEDAVG_NARROW_PART=1/2 objects defined each symbol twice and the shared link failed; the
product's stand-alone server-step unit does not exist there either.  The list must follow what the sources know."""

import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nvflare_amd import _build as B  # noqa: E402

OLD_REV = "22c4d2a"  # round 4's final tree
GOLDEN = os.path.join(ROOT, "tests", "golden", "csrc_round4")


def _export(dst):
    """Round 4's nvflare_amd/csrc as compile_units reads it, from tests/golden/csrc_round4/ (no git history needed):
    the two sources whose split macros it looks for are stored as they were at OLD_REV, the others (FILES.txt: that
    revision's file list) only have to exist."""
    csrc = os.path.join(dst, "nvflare_amd", "csrc")
    os.makedirs(csrc)
    with open(os.path.join(GOLDEN, "FILES.txt")) as fh:
        names = fh.read().split()
    for name in names:
        stored = os.path.join(GOLDEN, name)
        if os.path.exists(stored):
            shutil.copy(stored, os.path.join(csrc, name))
        else:
            open(os.path.join(csrc, name), "w").close()
    assert os.path.getsize(os.path.join(csrc, B.EPI_SOURCE)) and os.path.getsize(os.path.join(csrc, B.NARROW_SOURCE))
    return csrc


def _check_unique(units):
    names = [u[1] for u in units]
    assert len(names) == len(set(names)), names
    # one object per (source, flags): no two units compile the same definitions
    keys = [(u[0], tuple(sorted(f for f in u[2] if not f.startswith("-DFEDAVG_EPI_FN2")))) for u in units]
    assert len(keys) == len(set(keys)), keys


def test_units_of_this_tree_are_split():
    units = B.compile_units(B.SOURCES, ab=False, csrc=B.CSRC)
    _check_unique(units)
    assert units == B.compile_units(B.SOURCES, ab=False)
    assert any("-DFEDAVG_EPI_PART=2" in u[2] for u in units) and any("-DFEDAVG_NARROW_PART=2" in u[2] for u in units)


@pytest.mark.parametrize("ab", [True, False])
def test_units_of_round4_sources_are_one_per_source(tmp_path, ab):
    csrc = _export(str(tmp_path))
    srcs = [s for s in B.SOURCES if os.path.exists(os.path.join(csrc, s))]
    units = B.compile_units(srcs, ab=ab, csrc=csrc)
    _check_unique(units)
    flags = [f for u in units for f in u[2]]
    assert not any("PART" in f for f in flags), flags
    assert not any(f == "-DFEDAVG_EPI_STEP" for f in flags)
    epi = [u for u in units if u[0] == B.EPI_SOURCE]
    assert len(epi) == len([u for u in (B.EPI_UNITS_AB if ab else B.EPI_UNITS) if u[1] is not None])
