"""CPU: the environment variables the Python package reads are a closed, documented list.  A route switch that is settled belongs in the code as a constant (the
tests flip it as a module attribute), not in the environment, where every variable is one more product variant nobody tests."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEPT = {"DCV_LIB_PATH", "DCV_PRECISION", "DCV_DP_OVERLAP", "DCV_MAX_ITERATIONS_AHEAD", "DCV_DEBUG_POISON", "DCV_NO_SIDE_STREAMS", "DCV_NO_WGRAD_SIDE",
        "DCV_NO_PACK_CACHE", "DCV_NO_HEAD_BN_DEFER"}
# os.environ.get("X" ...), os.environ["X"], os.environ.pop / setdefault("X" ...), "X" in os.environ, os.getenv("X" ...)
READ = re.compile(r"""os\.(?:environ(?:\.\w+)?\s*[\[(]|getenv\s*\()\s*["'](DCV_[A-Z0-9_]+)["']|["'](DCV_[A-Z0-9_]+)["']\s+(?:not\s+)?in\s+os\.environ""")


def test_environment_reads_are_the_documented_nine():
    files = sorted(glob.glob(os.path.join(ROOT, "dcvgan_amd", "*.py")))
    assert len(files) > 10
    read = {}
    for path in files:
        src = open(path).read()
        for m in READ.finditer(src):
            read.setdefault(m.group(1) or m.group(2), []).append(os.path.basename(path))
        # nothing reaches the environment by a route the pattern above does not see (an alias, a name put together at run time)
        assert len(re.findall(r"\benviron\b|\bgetenv\b", src)) == len(READ.findall(src)), f"{os.path.basename(path)}: an environment access this test cannot name"
    assert set(read) == KEPT, (sorted(set(read) - KEPT), sorted(KEPT - set(read)), read)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    missing = [n for n in sorted(KEPT) if not re.search(r"\b" + n + r"\b", doc)]
    assert not missing, f"not documented in INTEGRATION.md: {missing}"
