"""What tools/surface_mutants.py, emitter_mutants.py, vertex_mutants.py, head_mutants.py and bsdf_mutants.py share: scratch copies of the CPU oracle with one
deliberate error each (in a temporary directory: nothing of the tree is touched, and nothing is ever built for the device),
swapped in behind oracle.pg_oracle, the tests run against every copy, and the report of which tests catch the error.  A tool
keeps its MUTANTS (name, [(text of oracle/pg_oracle_render.c, its replacement[, how often the text occurs: 1])]), its TESTS
(test name, callable, argument tuple or None), its header text and its band()."""
import ctypes
import io
import os
import shutil
import subprocess
import sys
import tempfile
from contextlib import redirect_stdout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import pg_oracle as po  # noqa: E402

AS_IT_IS = "the oracle as it is"


def only():
    """the mutants' numbers on the command line (none: all of them, and the oracle as it is first)"""
    return [int(a) for a in sys.argv[1:] if not a.startswith("--")]


def build(tmp, number, edits):
    d = os.path.join(tmp, "oracle%d" % number)   # (a directory of its own: the loader knows a library by its path)
    os.makedirs(d)
    for f in os.listdir(os.path.join(ROOT, "oracle")):
        if f.endswith((".c", ".h")) or f == "Makefile":
            shutil.copy(os.path.join(ROOT, "oracle", f), d)
    p = os.path.join(d, "pg_oracle_render.c")
    s = open(p).read()
    for old, new, *times in edits:
        assert s.count(old) == (times[0] if times else 1), old
        s = s.replace(old, new)
    open(p, "w").write(s)
    subprocess.run(["make", "-C", d, "-s"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(d, "libpg_oracle.so"))
    po._declare(lib)
    return lib


def each_oracle(mutants):
    """-> the name of every oracle to report on, while oracle.pg_oracle uses it: the tree's own, then the chosen mutants"""
    chosen = only()
    with tempfile.TemporaryDirectory() as tmp:
        po.lib()
        own = po._lib
        if not chosen:
            yield AS_IT_IS
        for number, (name, edits) in enumerate(mutants):
            if chosen and number not in chosen:
                continue
            po._lib = build(tmp, number, edits)
            yield name
        po._lib = own


def run_tests(name, tests):
    """-> (name, the tests that fail, how many ran), and the block of the report"""
    failed, ran = [], 0
    for test, fn, args in tests:
        for a in args or (None,):
            ran += 1
            try:
                with redirect_stdout(io.StringIO()):
                    fn(*(() if a is None else (a,)))
            except Exception as e:   # (an AssertionError, or whatever a copy's nonsense raises further down)
                first = (str(e) or type(e).__name__).split("\n")[0]
                failed.append(("%s[%s]" % (test, a) if a is not None else test, first[:150]))
    print("== %s" % name)
    for t, why in failed:
        print("   FAILS %-75s %s" % (t, why))
    if not failed:
        print("   all %d tests pass" % ran)
    return name, [t for t, _ in failed], ran


def summary(lines, width=60):
    """lines: (name, what caught it or "") per oracle reported on"""
    print("== summary")
    for name, caught in lines:
        print("   %-*s %s" % (width, name, caught or "NOTHING FAILS" + ("" if name == AS_IT_IS else ": ESCAPES")))
    escaped = [name for name, caught in lines if not caught and name != AS_IT_IS]
    print("   escaped: %s" % (", ".join(escaped) if escaped else "none"))


def mutations(header, mutants, tests):
    print(header)
    results = [run_tests(name, tests) for name in each_oracle(mutants)]
    summary([(name, "caught by %d of %d tests: %s" % (len(failed), ran, ", ".join(failed[:3]) + (" ..." if len(failed) > 3 else "")) if failed else "")
             for name, failed, ran in results])


def worst_ratios(worst, band_c):
    print("worst ratio, C = 4 x it, and the committed BAND_C:")
    for k in sorted(worst):
        print("   %-8s %.3f   %.2f   %.2f" % (k, worst[k], 4 * worst[k], band_c[k]))


def main(header, mutants, tests, band):
    band() if "--band" in sys.argv else mutations(header, mutants, tests)
