"""The command line's transcript: a fixed list of `tomahawk` invocations that end while the options are parsed or at the absent input -
none reaches a device - and, per invocation, argv, exit code, stdout and stderr.

    python tests/golden/make_golden_cli_transcript.py <path to tomahawk> [out.json]

writes tests/golden/cli_transcript.json (or out.json): one line per distinct outcome - exit code, stdout, stderr - with every argv that
ends in it.  tests/test_cli_transcript.py runs the same list against the current build and
compares.  The fixture is recorded from the commit BEFORE a change to the command layer, never from the code under test.  Needs nothing
but the executable's path: the host library is not loaded into Python.

Three things are normalised before storing and before comparing, nothing else: the executable's own path, which getopt prints, becomes
`tomahawk`; the banner's `Libraries:` line, which carries the machine's zstd version, becomes a fixed token; and so does the wall-clock
time in brackets with which the host library begins each of its lines once a command has got as far as opening its input."""
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "cli_transcript.json")

ENGINE_COMMANDS = ("calc", "ldscore", "prune", "clump", "ldmatrix", "lddecay", "ldaggregate", "relationship")
IN = ["-i", "absent.twk"]
# what a command needs besides -i to get as far as the input
NEEDS = {"calc": ["-o", "out"], "clump": ["-a", "absent.assoc"], "ldmatrix": ["-o", "out"]}
# every command-specific flag of the reduce commands: (short, long, takes an argument)
OWN_FLAGS = (("a", "assoc", True), ("1", "p1", True), ("2", "p2", True), ("s", "stat", True), ("f", "fill", True), ("T", "text", False),
             ("d", "range", True), ("b", "bins", True), ("x", "xbins", True), ("y", "ybins", True), ("R", "reduce", True), ("m", "minCount", True))
SHARED_BAD = (["-t", "0"], ["-t", "abc"], ["-c", "0"], ["-C", "0"], ["-r", "-1"], ["-r", "2"], ["-P", "-1"], ["-P", "0.5"], ["-P", "2"],
              ["-w", "abc"], ["-w", "0"], ["-w", "1e"], ["--threads=0"], ["--minR2=2"], ["--minP=0.5"],
              ["--windowBases=abc"], ["--engine-option", "x"], ["--engine-option", "=1"], ["--engine-option", "x="])
SHARED_GOOD = (["-t", "2"], ["-c", "3", "-C", "1"], ["-r", "1"], ["-P", "1"], ["-w", "1e3"], ["-p", "-u"], ["-I", "1:100-200", "-I", "2"],
               ["--engine-option", "fused=0", "--engine-option", "three=2"], ["--force-phased"], ["--input=other.twk"], ["-o", "-"])
OWN = {
    "calc": (["-b", "0"], ["-b", "5"], ["-k", "3"], ["-m"], ["-M"], ["--low-memory"], ["--bitmaps"], ["--block-size=0"], ["--block-size=7"],
             ["--compression-level=2"], ["--cross-chr-only"], ["--no-cross-chr"], ["-X"], ["-x"], ["-S", "list"], ["--samples=list"], ["-a", "1"],
             ["-A", "1"], ["-s"], ["-d"], ["--silent"], ["--detailedProgress"], ["--low-memory", "1"], ["--bitmaps", "1"], ["--samples", "list"], ["-P", "0"], ["-P", "0.5", "-r", "0.3"]),
    "ldscore": (),
    "prune": (),
    "clump": (["-1", "abc"], ["-1", "-0.1"], ["-1", "1.5"], ["-1", "0.5x"], ["-1", "nan"], ["-2", "abc"], ["-2", "-0.1"], ["-2", "1.5"], ["-1", "0"], ["-1", "1", "-2", "1"],
              ["-2", "0", "-1", "0"], ["-2", "1"], ["-1", "0.5", "-2", "0.1"], ["-2", "0.1", "-1", "0.5"], ["--p1=2"], ["--p2=2"], ["--p1=1e-8", "--p2=1e-3"],
              ["--assoc=other.assoc"]),
    "ldmatrix": (["-s", "x"], ["-s", ""], ["-s", "R2"], ["-s", "r"], ["-s", "r2"], ["-s", "D"], ["-s", "Dprime"], ["--stat=dprime"], ["--stat=D"],
                 ["-f", "abc"], ["-f", "0.5x"], ["-f", ""], ["-f", "nan"], ["-f", "inf"], ["-f", "-7"], ["-f", "1e-3"], ["--fill=x"], ["--fill=2"],
                 ["-T"], ["--text"], ["-o", "-"], ["-o", ""]),
    "lddecay": (["-d", "abc"], ["-d", "-1"], ["-d", "0"], ["-d", "1", "-b", "1"], ["-d", "4294967295"], ["-d", "4294967296"], ["-d", "1e3"], ["-d", "1e10"], ["-d", "1.5"],
                ["-b", "x"], ["-b", "0"], ["-b", "1"], ["-b", "4096"], ["-b", "4097"], ["-b", "1e2"], ["-b", "1e4"], ["--range=0"], ["--bins=0"],
                ["--range=5000", "--bins=50"], ["-d", "10", "-b", "100"], ["-b", "100", "-d", "10"], ["-d", "100", "-b", "100"], ["-d", "999"],
                ["-w", "500"], ["-w", "1000"], ["-w", "5000"], ["-w", "500", "-b", "500"], ["-w", "500", "-d", "2000"], ["-d", "2000", "-w", "500"],
                ["-d", "0", "-b", "0"], ["-b", "0", "-d", "0"], ["-d", "x", "-b", "y"], ["-b", "y", "-d", "x"]),
    "ldaggregate": (["-x", "abc"], ["-x", "0"], ["-x", "1"], ["-x", "4096"], ["-x", "4097"], ["-x", "1e2"], ["-x", "-3"], ["-y", "abc"], ["-y", "0"], ["-y", "1"],
                    ["-y", "4096"], ["-y", "4097"], ["-y", "1e9"], ["-m", "abc"], ["-m", "-1"], ["-m", "0"], ["-m", "9007199254740992"], ["-m", "1e16"], ["-m", "1e3"],
                    ["--xbins=0"], ["--ybins=0"], ["--minCount=x"], ["--xbins=10", "--ybins=20", "--minCount=1"],
                    ["-R", "mean"], ["-R", "count"], ["-R", "n"], ["-R", "min"], ["-R", "max"], ["-R", "sd"], ["-R", "total"], ["-R", "median"], ["-R", ""],
                    ["--reduce=sum"], ["--reduce=sd"], ["-s", "r"], ["-s", "r2"], ["-s", "D"], ["-s", "Dprime"], ["-s", "x"], ["-s", ""], ["--stat=king"],
                    ["-x", "0", "-y", "0"], ["-y", "0", "-x", "0"], ["-R", "bad", "-s", "bad"], ["-s", "bad", "-R", "bad"]),
    "relationship": (["-s", "ibs"], ["-s", "ibs0"], ["-s", "king"], ["-s", "KING"], ["-s", "ibs1"], ["-s", ""], ["-s", "r2"], ["--stat=x"], ["--stat=ibs"],
                     ["-f", "abc"], ["-f", "0.5x"], ["-f", ""], ["-f", "nan"], ["-f", "-7"], ["--fill=x"], ["--fill=0"], ["-T"], ["--text"], ["-T", "-o", "-"],
                     ["-o", "out", "-T"], ["-o", "out"], ["--output=out", "--text"], ["-t", "0"], ["-t", "x"], ["--threads=0"], ["--threads", "0"], ["--threads", "3"],
                     ["--interval", "1:5-9"], ["-I", "1", "-I", "2"], ["--engine-option", "x"], ["--engine-option", "=1"], ["--engine-option", "x="],
                     ["--engine-option", "a=1", "--engine-option", "b=2"],
                     ["-p"], ["-u"], ["-r", "0.2"], ["-w", "1000"], ["-c", "3"], ["-C", "1"], ["-P", "1"], ["-P", "0.5"], ["--force-phased"], ["--force-unphased"],
                     ["--minR2", "0.2"], ["--minR2=0.2"], ["--windowBases", "1000"], ["--parts", "3"], ["--partStart", "1"], ["--minP", "1"], ["--minR2"],
                     ["-s", "bad", "-f", "bad"], ["-f", "bad", "-s", "bad"], ["-p", "-s", "bad"], ["-s", "bad", "-p"], ["-T", "-f", "bad"], ["-w", "x", "-T"]),
}
# two things wrong at once, in both orders; and what is checked after the options against what is checked among them
PAIRS = (["-t", "0"], ["-r", "2"], ["-c", "0"], ["--assoc=x"])
AFTER = {
    "calc": ([], ["-i", "absent.twk"], ["-o", "out"], ["-o", "out", "-t", "0"]),
    "ldscore": ([], ["-t", "0"], ["-o", "out"]),
    "prune": ([], ["-c", "3"], ["-o", "out"]),
    "clump": ([], ["-i", "absent.twk"], ["-a", "absent.assoc"], ["-1", "0.5", "-2", "0.1"], ["-i", "absent.twk", "-1", "0.5", "-2", "0.1"],
              ["-a", "absent.assoc", "-1", "0.5", "-2", "0.1"], ["-i", "absent.twk", "-1", "2"]),
    "ldmatrix": ([], ["-i", "absent.twk"], ["-o", "out"], ["-o", "-", "-i", "absent.twk"], ["-i", "absent.twk", "-s", "x"], ["-s", "r2"]),
    "lddecay": ([], ["-d", "10", "-b", "100"], ["-w", "500"], ["-i", "absent.twk", "-w", "500", "-t", "0"]),
    "ldaggregate": ([], ["-x", "10"], ["-x", "0"]),
    "relationship": ([], ["-T"], ["-o", "out", "-T"], ["-i", "absent.twk", "-T"], ["-T", "-p"]),
}


def invocations():
    """The fixed list: one argv (without the executable) per entry."""
    out = [[], ["--version"], ["version"], ["--help"], ["help"], ["no-such-command"], ["no-such-command", "-i", "x"], ["Calc"],
           ["import"], ["scalc"], ["calc-single"], ["sort"], ["view"], ["concat"], ["concatenate"], ["scalc", "-i", "absent.twk", "-t", "0"]]
    for cmd in ENGINE_COMMANDS:
        base = [cmd] + IN + NEEDS.get(cmd, [])
        out.append([cmd])
        out.append([cmd, "-i"])                                # (argc < 3 is the usage's only test)
        out.append(base)                                       # well-formed, the input is absent
        out.append([cmd] + NEEDS.get(cmd, []) + IN)
        for flags in SHARED_BAD + SHARED_GOOD:
            out.append(base + list(flags))
        for flags in OWN[cmd]:
            out.append(base + list(flags))
        if cmd != "relationship":                              # a long name whose argument is optional, the value as the next word: no argument
            out += [base + ["--windowBases", "1000"], base + ["--interval", "1:5-9"], base + ["--windowBases", "1000", "-t", "0"], base + ["-t", "0", "--interval", "1:5-9"]]
        for short, long_name, has_arg in OWN_FLAGS:            # every command-specific flag on every command: long (the guards tell them apart), short
            out.append(base + ["--" + long_name + ("=1" if has_arg else "")])
            if cmd == "calc" or short in "asR":                # (a short flag that is not in the command's getopt string is getopt's '?', whichever it is)
                out.append(base + ["-" + short] + (["1"] if has_arg else []))
        for flags in (["-Z"], ["-?"], ["--no-such-option"], ["stray", "-t", "0"], ["--", "-t", "0"]):
            out.append(base + flags)
        for flag in ("-i", "-t", "--engine-option", "--input", "-s", "-d"):
            out.append(base + [flag])                          # the last word lacks its argument
        for k, first in enumerate(PAIRS):
            for second in PAIRS[k + 1:]:
                out.append(base + first + second)
                out.append(base + second + first)
        for flags in AFTER[cmd]:
            out.append([cmd] + list(flags))
    seen, unique = set(), []
    for argv in out:
        if tuple(argv) not in seen:
            seen.add(tuple(argv))
            unique.append(argv)
    return unique


def normalise(text, cli):
    text = text.replace(cli, "tomahawk")
    text = re.sub(r"^Libraries: .*$", "Libraries: <LIBRARIES>", text, flags=re.M)
    return re.sub(r"^\[\d{4}-\d\d-\d\d \d\d:\d\d:\d\d,\d{3}\]", "[<TIME>]", text, flags=re.M)


def run_one(cli, argv, cwd):
    r = subprocess.run([cli] + argv, cwd=cwd, stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
    return tuple(argv), (r.returncode, normalise(r.stdout.decode("utf-8", "replace"), cli), normalise(r.stderr.decode("utf-8", "replace"), cli))


def record(cli, jobs=8):
    """Every invocation of the list run with `cli` in an empty directory of its own -> {argv: (exit, stdout, stderr)}, in the list's order."""
    cli = os.path.abspath(cli)
    with tempfile.TemporaryDirectory() as cwd:
        with ThreadPoolExecutor(jobs) as pool:
            got = dict(pool.map(lambda argv: run_one(cli, argv, cwd), invocations()))
        left = sorted(os.listdir(cwd))
    assert not left, "an invocation wrote a file: %s" % left
    return got


def load(path=FIXTURE):
    """The fixture as record() returns a transcript."""
    with open(path) as f:
        return {tuple(argv): (o["exit"], o["stdout"], o["stderr"]) for o in json.load(f) for argv in o["argv"]}


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    transcript = record(sys.argv[1])
    outcomes = {}
    for argv, outcome in transcript.items():
        outcomes.setdefault(outcome, []).append(list(argv))
    with open(sys.argv[2] if len(sys.argv) > 2 else FIXTURE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps({"exit": o[0], "stdout": o[1], "stderr": o[2], "argv": argvs}) for o, argvs in outcomes.items()) + "\n]\n")
    print("%d invocations recorded, %d distinct outcomes" % (len(transcript), len(outcomes)))
