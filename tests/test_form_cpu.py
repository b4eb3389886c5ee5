"""Who may take which form of a count launch (csrc/hip/ld_form.h), without a GPU: `make form-check` - decide_form over every combination of
the facts a plan, a cut-off and the options fix and of the grants a launch's owner gives, and what a launch's outcome takes from the running
call (CallForms::gave_up); the named grants against the expressions they replaced, the thresholds at their edges, and the sample ladder
(decide_wants) under scripted samplers - under AddressSanitizer and UBSan."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_forms_grants_and_what_a_call_gives_up_on_the_cpu():
    """No two forms that exclude each other, a reducing launch in none, every form only under its grants and options, no grant whose
    withdrawal adds a form (two -> three excepted); a list that overflowed or a launch too rich in candidates ends exactly its own forms
    for the call, never one the launch was not granted, and telling the call twice changes nothing; the sample ladder keeps its invariants
    over every option, fact, plan length and sample outcome, and its named scripts take the samples and end in the wants written out."""
    r = subprocess.run(["make", "-C", ROOT, "form-check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    m = re.search(r"form-check: (\d+) cases, (\d+) bad", r.stdout)
    assert m and int(m.group(1)) >= 2_000_000 and int(m.group(2)) == 0, r.stdout[-2000:]
