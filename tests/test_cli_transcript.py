"""The command line, byte for byte: every invocation of tests/golden/make_golden_cli_transcript.py - usage texts, refusals, getopt's own
complaints, two errors at once in both orders, a well-formed line as far as the absent input - run with the current build and compared
with tests/golden/cli_transcript.json, which the commit before the command layer was reshaped recorded.  No invocation reaches a device."""
from tests.golden import make_golden_cli_transcript as transcript
from tomahawk_amd import hostlib


def test_every_invocation_prints_and_exits_as_recorded():
    want = transcript.load()
    got = transcript.record(hostlib.CLI_PATH)
    assert sorted(got) == sorted(want) == sorted(tuple(a) for a in transcript.invocations()), "the list of invocations and the fixture differ: record it again from the parent commit"
    different = [argv for argv in want if want[argv] != got[argv]]
    for argv in different[:5]:
        print("argv:", list(argv))
        for key, w, g in zip(("exit", "stdout", "stderr"), want[argv], got[argv]):
            if w != g:
                print("  %s recorded: %r\n  %s now:      %r" % (key, w, key, g))
    assert not different, "%d of %d invocations differ from the recorded transcript" % (len(different), len(want))


def test_the_list_covers_every_command_and_names_no_device():
    """What the fixture is for: each of the eight engine commands bare, well-formed, with a foreign flag short and long, with two errors in
    both orders; and nothing in any recorded stream says that an output was opened or an input unpacked."""
    want = transcript.load()
    argvs = [list(a) for a in want]
    assert len(argvs) >= 700
    for cmd in transcript.ENGINE_COMMANDS:
        assert [cmd] in argvs and [cmd, "-i", "absent.twk"] + transcript.NEEDS.get(cmd, []) in argvs
        mine = [a for a in argvs if a and a[0] == cmd]
        assert any("--assoc=1" in a for a in mine) and any("-R" in a for a in mine) and any("-Z" in a for a in mine)
        assert any(a[-4:] == ["-t", "0", "-r", "2"] for a in mine) and any(a[-4:] == ["-r", "2", "-t", "0"] for a in mine)
    decay = [a[1:] for a in argvs if a and a[0] == "lddecay"]
    assert ["-i", "absent.twk", "-d", "10", "-b", "100"] in decay and ["-i", "absent.twk", "-b", "100", "-d", "10"] in decay and ["-i", "absent.twk", "-w", "500"] in decay
    for argv, (code, out, err) in want.items():
        assert "Unpacking" not in err and "[WRITER]" not in err and "hip error" not in err.lower(), argv
        assert code in (0, 1), argv
