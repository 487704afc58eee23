"""pak_io.c, the unit of the tools' host library that reads and writes the users' files: it needs no GPU library, so it
is built alone here -- and run under AddressSanitizer and UBSan, as a stand-alone program, on every golden file."""
import glob
import os
import subprocess

from conftest import GOLDEN, ROOT

HOST = os.path.join(ROOT, "som_lvq_pak_amd", "host")
HELPERS = os.path.join(ROOT, "tests", "helpers")
INC = ["-I", HOST, "-I", os.path.join(ROOT, "include")]
PAK_IO = os.path.join(HOST, "pak_io.c")
# the runtimes are linked into the program, so it does not depend on its place in the process's list of libraries
SANITIZED = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")      # the label table lives as long as the process, by design


def build(exe, helper, flags):
    subprocess.check_call(["gcc", *flags, *INC, "-o", str(exe), os.path.join(HELPERS, helper), PAK_IO, "-lm"])
    return str(exe)


def undefined_symbols(obj):
    out = subprocess.run(["nm", "-u", str(obj)], stdout=subprocess.PIPE, text=True, check=True).stdout
    return [line.split()[-1] for line in out.splitlines() if line.strip()]


def test_pak_io_needs_no_gpu_library(tmp_path):
    """neither built as the tools build it nor built plain does pak_io.o ask for a somhip_* or hip* symbol, and the
    number-parser check links against the plain object with -lm alone"""
    for name, flags in (("tools.o", ["-O2", "-Wall", "-ffp-contract=off", "-fopenmp"]), ("plain.o", ["-O2"])):
        obj = tmp_path / name
        subprocess.check_call(["gcc", *flags, *INC, "-c", "-o", str(obj), PAK_IO])
        syms = undefined_symbols(obj)
        assert syms and not [s for s in syms if "somhip_" in s or "hip" in s.lower()], syms
    exe = tmp_path / "parse_check"
    subprocess.check_call(["gcc", "-O2", *INC, "-o", str(exe), os.path.join(HELPERS, "parse_check.c"), str(tmp_path / "plain.o"), "-lm"])
    p = subprocess.run([str(exe), "20000"], stdout=subprocess.PIPE, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("mismatches 0"), p.stdout


def test_file_io_round_trips_clean_under_sanitizers(tmp_path):
    """tests/helpers/entries_roundtrip.c (open, text and fp32 round trips, pick_rows, the -rand shuffle, close) over all
    golden .dat and .cod files, a gen: source and a file with weights and fixed points: no failed check, the same
    report from the plain and the sanitized build, and not a word from the sanitizers; the number parser likewise"""
    files = sorted(glob.glob(os.path.join(GOLDEN, "data", "*.dat"))) + sorted(glob.glob(os.path.join(GOLDEN, "cli", "*.cod")))
    assert len(files) >= 20
    reports = {}
    for kind, flags, env in (("plain", ["-O2"], None), ("sanitized", SANITIZED, SAN_ENV)):
        work = tmp_path / kind
        work.mkdir()
        exe = build(work / "entries_roundtrip", "entries_roundtrip.c", flags)
        p = subprocess.run([exe] + files, cwd=work, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0, (kind, p.stdout[-2000:], p.stderr[-4000:])
        assert p.stdout.strip().endswith("failed checks 0") and "FAILED" not in p.stdout, p.stdout
        reports[kind] = p
    assert reports["plain"].stdout == reports["sanitized"].stdout
    assert reports["sanitized"].stderr == ""
    # every file was opened at least without labels, and the sources without a file too
    for name in [os.path.basename(f) for f in files] + ["gen:k=3,dim=5,n=40,seed=9,labels=1", "made_here.dat"]:
        assert ("%s labels_needed 0: dim " % name) in reports["plain"].stdout, name
    exe = build(tmp_path / "parse_check", "parse_check.c", SANITIZED)
    p = subprocess.run([exe, "20000"], env=SAN_ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("mismatches 0") and p.stderr == "", (p.stdout, p.stderr)
