"""The BSGPU_* environment switches of libbsgpu, kept honest from the source text alone: one header reads the environment, the
switch table in docs/SWITCHES.md lists exactly the switches the code reads, every one of them is named by a test (the three timing
probes apart), and the switches that were pruned stay pruned."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "beam_slam_amd", "csrc")
ENV_HEADER = "bsgpu_env.h"
SOURCE_SUFFIXES = (".h", ".cpp", ".hip", ".py", ".sh", ".c", ".txt", ".md")
# timing probes: the same kernels with wall-clock stamps, read by scripts/chol_probe.py, scripts/chol_chains.py and friends — no alternative path to test
PROBES = {"BSGPU_CHOL_PROBE", "BSGPU_BACKSOLVE_PROBE", "BSGPU_PCG_PROBE"}
# off-switches of A/Bs the default won, removed with the branches they selected
PRUNED = ["BSGPU_LM_DEVICE_NOWAIT", "BSGPU_LM_DEVICE_ARGS", "BSGPU_CAND_ONE_PASS", "BSGPU_BAND_LOWER", "BSGPU_CHOL_ROWS", "BSGPU_BATCH_BULK",
          "BSGPU_BATCH_ONE_PASS", "BSGPU_BATCH_THREADS", "BSGPU_CHOL_SPLIT", "BSGPU_DIM_T_STEP3", "BSGPU_DIM_MERGE", "BSGPU_DIM_T_CHAIN0",
          "BSGPU_DIM_T_HOP", "BSGPU_DIM_T_HOP_TILE", "BSGPU_DIM_CANDIDATES"]


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _files(top, suffixes=SOURCE_SUFFIXES):
    for d, dirs, names in os.walk(top):
        dirs[:] = [x for x in dirs if x != "__pycache__"]
        for n in names:
            if n.endswith(suffixes) or n == "Makefile":
                yield os.path.join(d, n)


def _switches_read():
    """the names the library hands to the helpers of bsgpu_env.h: every "BSGPU_..." string literal under csrc/"""
    names = set()
    for path in _files(CSRC, (".h", ".cpp", ".hip")):
        names |= set(re.findall(r'"(BSGPU_[A-Z0-9_]+)"', _read(path)))
    return names


def test_one_header_reads_the_environment():
    readers = sorted(os.path.basename(p) for p in _files(CSRC) if "getenv" in _read(p))
    assert readers == [ENV_HEADER]


def test_switch_table_lists_what_the_code_reads():
    table = set(re.findall(r"^\| `(BSGPU_[A-Z0-9_]+)", _read(os.path.join(ROOT, "docs", "SWITCHES.md")), re.M))
    read = _switches_read()
    assert len(read) == 44
    assert table == read, (sorted(table - read), sorted(read - table))


def test_every_switch_is_named_by_a_test():
    here = os.path.abspath(__file__)
    text = "\n".join(_read(p) for p in _files(os.path.join(ROOT, "tests")) if os.path.abspath(p) != here)
    read = _switches_read()
    assert PROBES <= read
    unnamed = sorted(n for n in read - PROBES if not re.search(n + r"\b", text))
    assert unnamed == []


def test_pruned_switches_stay_pruned():
    here = os.path.abspath(__file__)
    found = []
    for top in ("beam_slam_amd", "include", "tests", "scripts"):
        for p in _files(os.path.join(ROOT, top)):
            if os.path.abspath(p) == here:
                continue
            text = _read(p)
            found += [(os.path.relpath(p, ROOT), n) for n in PRUNED if re.search(n + r"\b", text)]
    assert found == []
