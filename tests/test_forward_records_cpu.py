"""Three properties of the forward's optional records over the full crossing of tests/forward_records.py - every plan flavour
with every value of every record, at each entry point over the records that entry point takes.  No GPU: every plan has
workspace = NULL, so a call that passes every other refusal ends at the workspace-size refusal and nothing is launched."""
import re

import forward_records as fr
from rajni_amd import _native as nat

LEVELS = range(len(fr.ENTRY_POINTS))


def test_a_null_trailing_record_is_the_next_narrower_entry_point():
    """Delegation: entry point k on its records and entry point k + 1 on the same records plus a NULL one give the same return
    code and the same refusal text (which names entry point k where it names one); so do the size functions' returns."""
    lib = nat.lib()
    calls = 0
    for level in LEVELS[:-1]:
        for case in fr.cases(level):
            narrow, wide = fr.forward(lib, level, case), fr.forward(lib, level, case, extra_null=1)
            assert narrow == wide, (fr.ENTRY_POINTS[level], [v.label for v in case], narrow, wide)
            calls += 1
    assert calls > 700000, calls      # the whole crossing ran: 11 * (1 + 17 + 17 * 9 + ...)
    for level in range(len(fr.SIZE_FUNCTIONS) - 1):
        for case in fr.size_cases(level):
            narrow, wide = fr.size(lib, level, case), fr.size(lib, level, case, extra_null=1)
            assert narrow == wide, (fr.SIZE_FUNCTIONS[level], [v.label for v in case], narrow, wide)


def test_the_size_function_and_the_forward_agree_on_the_byte_count():
    """Every combination of valid values that the headers make legal passes every refusal of the forward but the last, and the
    size that refusal asks for is what the matching size function returned.  A condition, not a sample: no legal combination
    is skipped."""
    lib = nat.lib()
    top = len(fr.ENTRY_POINTS) - 1
    seen = 0
    for case in fr.cases(top, only_valid=True):
        if not fr.legal(*case):
            continue
        plan, ext, prefix, layers, image, query, pool = case
        want = fr.size(lib, len(fr.SIZE_FUNCTIONS) - 1, (plan, prefix, image, query, pool))
        rc, msg = fr.forward(lib, top, case)
        m = re.fullmatch(rb"rajni_vit_forward: workspace too small \(0 < (\d+)\)", msg)
        assert rc == 1 and m, ([v.label for v in case], rc, msg)
        assert int(m.group(1)) == want and want > 0, ([v.label for v in case], msg, want)
        seen += 1
    assert seen >= 100, seen


def test_every_invalid_value_is_refused_under_its_record_s_name():
    """Each invalid value beside otherwise-default records (the plain plan, NULL for every other record), at the entry point
    that takes its record: a non-zero return code and a message that names the record's entry point or the field."""
    lib = nat.lib()
    ax = fr.axes()
    default = [ax["plan"][0]] + [ax[name][0] for name in fr.RECORDS]
    assert all(v.valid for v in default) and default[0].label == "plain" and all(v.obj is None for v in default[1:])
    checked = 0
    for level, name in enumerate(("plan",) + fr.RECORDS):
        for value in ax[name]:
            if value.valid:
                continue
            case = default[:level] + [value]
            rc, msg = fr.forward(lib, level, case)
            assert rc != 0 and value.needles and any(n.encode() in msg for n in value.needles), (name, value.label, rc, msg)
            checked += 1
    assert checked == sum(not v.valid for vals in ax.values() for v in vals) and checked >= 25, checked
