"""The library's run-time switches: the environment variables csrc/ reads are exactly the comparator and diagnostic knobs that tests, bench.py and the tools use,
and README.md's table lists exactly those. A knob added for an experiment has to be added here and documented, or taken out again when the experiment is over."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rnb-neus2_amd", "csrc")

KNOBS = {
    "RNB_SCATTER_PLAIN", "RNB_GRID_PRESORT", "RNB_MARCH_NARROW", "RNB_MARCH_NARROW_FROM", "RNB_FWD_K1", "RNB_FWD_BWD_GENERIC", "RNB_MARCH_SKIP", "RNB_MARCH_SKIP_NARROW",
    "RNB_MARCH_BBOX", "RNB_LOSS_WAVE_PER_RAY", "RNB_LOSS_CHAIN_RECORDS", "RNB_LOSS_FLAT", "RNB_LOSS_SCAN_FUSED", "RNB_DW_SLICED", "RNB_DP_FORCE_COLLECTIVES",
    "RNB_DETERMINISTIC", "RNB_MARCH_STATS",
}


def getenv_names():
    """The string arguments of every getenv( in csrc/, and the number of calls."""
    names, calls = [], 0
    for f in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, f), encoding="utf-8").read()
        calls += len(re.findall(r"\bgetenv\s*\(", text))
        names += re.findall(r"\bgetenv\s*\(\s*\"([^\"]*)\"", text)
    return names, calls


def readme_table_names():
    text = open(os.path.join(ROOT, "README.md"), encoding="utf-8").read()
    section = text.split("## Environment switches", 1)[1].split("\n## ", 1)[0]
    rows = [line for line in section.splitlines() if line.startswith("| `")]
    return [re.match(r"\| `([A-Z0-9_]+)", line).group(1) for line in rows]


def test_the_library_reads_the_kept_knobs_and_no_others():
    names, calls = getenv_names()
    assert len(names) == calls, "a getenv call whose variable is not a string literal escapes this list"
    assert set(names) == KNOBS, {"not read any more": sorted(KNOBS - set(names)), "new": sorted(set(names) - KNOBS)}
    assert calls <= len(KNOBS) + 1, calls  # RNB_FWD_BWD_GENERIC is read twice (the half mode refuses it at creation)


def test_readme_lists_exactly_the_knobs_the_library_reads():
    listed = readme_table_names()
    assert len(listed) == len(set(listed)), listed
    assert set(listed) == KNOBS, {"missing from README": sorted(KNOBS - set(listed)), "listed but not read": sorted(set(listed) - KNOBS)}
