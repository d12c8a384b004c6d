"""The library's runtime switches: the C sources read exactly the six environment variables that tests set, INTEGRATION.md documents each
of them, and the names of the switches that left the library are gone from the product tree and its documents (no compiler, no GPU)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RUNTIME = {"GSPN_BALL_CELLS", "GSPN_BALL_PREFIX", "GSPN_FWD_SHORT_MT", "GSPN_FWD_SHORT_NT", "GSPN_FWD_LEAN_BN", "GSPN_MFMA_SPLIT"}

# switches of the closed sweeps; the tunable numbers that became build-time constants keep their names as macros and are not listed
REMOVED = ["GSPN_WGRAD_FORCE", "GSPN_WGRAD_LEAN", "GSPN_PREAGG_U", "GSPN_PREAGG_FWD16", "GSPN_PREAGG_BLOCKS", "GSPN_CSR_WIDE", "GSPN_CSR_GATHER16",
           "GSPN_FWD_LEAN", "GSPN_FWD_NO_STREAM", "GSPN_FWD_SHORT", "GSPN_FWD_FORCE_BN", "GSPN_BWD_FORCE_BN",
           "GSPN_BWD_LEAN", "GSPN_BWD_LEAN_BN", "GSPN_BWD_FUSED", "GSPN_BWD_FUSED_BPC", "GSPN_NN_WAVE", "GSPN_NN_CELLS", "GSPN_NN_GRID",
           "GSPN_CSR_GLOBAL", "GSPN_CSR_SLICES", "GSPN_FPS_BIN_SLICES", "GSPN_NMGRAD_LDS", "GSPN_GEOM_CLAIM_LDS"]


def _read(path):
    with open(path, errors="replace") as fh:
        return fh.read()


def _csrc():
    return sorted(glob.glob(os.path.join(ROOT, "gspn_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "gspn_amd", "csrc", "*.h")))


def test_the_library_reads_exactly_the_six_documented_switches():
    read = set()
    for path in _csrc():
        read |= set(re.findall(r'\b(?:getenv|env_int)\(\s*"(GSPN_[A-Z0-9_]+)"', _read(path)))
        # a name handed to getenv / env_int through a variable would escape the pattern above: there is no such call
        assert not re.search(r'\b(?:getenv|env_int)\(\s*[^"\s]', re.sub(r"static inline int env_int\(const char\* name, int dflt\).*", "", _read(path))), path
    assert read == RUNTIME
    doc = _read(os.path.join(ROOT, "INTEGRATION.md"))
    for name in sorted(RUNTIME):
        assert re.search(r"\b%s\b" % name, doc), name


def test_the_removed_switches_are_named_nowhere_in_the_product():
    paths = [os.path.join(ROOT, "INTEGRATION.md"), os.path.join(ROOT, "README.md")]
    for top in ("gspn_amd", "include"):
        for d, dirs, files in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [x for x in dirs if x not in ("build", "lib", "__pycache__")]
            paths += [os.path.join(d, f) for f in files if f.endswith((".hip", ".h", ".py", ".md"))]
    assert len(paths) > 40
    # whole names only: GSPN_FWD_SHORT_MT, GSPN_FWD_LEAN_BN and GSPN_GEOM_CLAIM_LDS_DEFAULT stay
    pat = re.compile(r"\b(%s)\b" % "|".join(REMOVED))
    found = [(os.path.relpath(p, ROOT), m.group(1)) for p in paths for m in pat.finditer(_read(p))]
    assert not found, found
