"""The launch plans of csrc/conv_igemm.hip (forward, eval-fused forward and every data-gradient form: tile, ROW3, FAST, tile and
group counts, the merged four-class launch, the BatchNorm-backward slot counts, the folded-form threshold) against
tests/golden/conv_plans.json.gz, row for row, under the default environment and under every dispatch knob (tools/wgrad_plans.py
records and evaluates the table; it was recorded from the library before conv_plan() existed).  No GPU: the queries read no pointer
and launch nothing.  The launcher, the slot queries and the plan query read one plan; engine/buffers.py sizes the partial buffers
from the slot queries, so the tests below also pin the relations between the queries and that each *_bnred launcher needs exactly the
slot count its query answers.  A deliberate change of a rule: python tools/wgrad_plans.py --record-conv tests/golden/conv_plans.json.gz
and review the diff of the file."""
import ctypes as C
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_plans.json.gz")
_spec = importlib.util.spec_from_file_location("wgrad_plans", os.path.join(ROOT, "tools", "wgrad_plans.py"))
wp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(wp)

ANSWER = ("rc", "bm", "bn", "row3", "fast", "tiles_m", "tiles_n", "groups_m", "merged", "slots")


@pytest.fixture(scope="module")
def built():
    from object_detection_cib_amd import build
    return build.build(verbose=False)


@pytest.fixture(scope="module")
def table():
    return wp.load_table(GOLDEN)


@pytest.mark.parametrize("setting", list(wp.CONV_SETTINGS))
def test_library_reproduces_recorded_plans(built, table, setting):
    """one child process per knob setting (a knob is read once per process)"""
    assert table["settings"][setting]["env"] == wp.CONV_SETTINGS[setting]
    want_conv, want_fold = wp.expected(table, setting)
    got_conv, got_fold = wp.run_setting(setting, GOLDEN)
    rows = wp.conv_rows(table)
    assert len(got_conv) == len(rows) == len(want_conv) and len(got_fold) == len(table["fold"]) == len(want_fold)
    bad = [(rows[i], dict(zip(ANSWER, g)), dict(zip(ANSWER, w))) for i, (g, w) in enumerate(zip(got_conv, want_conv)) if g != w]
    assert not bad, "%d conv rows differ under %s; (row, got, recorded) of the first: %s" % (len(bad), setting, bad[:3])
    bad = [(r, g, w) for r, g, w in zip(table["fold"], got_fold, want_fold) if g != w]
    assert not bad, "%d fold rows differ under %s; (row, got, recorded) of the first: %s" % (len(bad), setting, bad[:3])


def test_table_is_self_consistent_and_covers_the_hand_cases(table):
    """The relations between the queries in every recorded row under every setting (a refusing query records its return code
    alone), every knob moves something, and the hand cases and boundaries each have a row."""
    rows = wp.conv_rows(table)
    assert list(table["settings"]) == list(wp.CONV_SETTINGS)
    for name in wp.CONV_SETTINGS:
        conv, _ = wp.expected(table, name)
        for r, a in zip(rows, conv):
            if a[0] != 0:
                assert len(a) == 1 and a[0] < 0, (name, r, a)
                continue
            op, got = r[14], dict(zip(ANSWER, a))
            want = {0: got["slots"],                                        # op 0 is an upper bound, checked below
                    1: got["groups_m"] if got["fast"] else 0,
                    2: 4 * got["groups_m"] if got["merged"] else 0,
                    3: 4 * got["groups_m"],
                    4: got["groups_m"]}[op]
            if op == 0:
                assert got["groups_m"] <= got["slots"], (name, r, got)
            elif "KODHIP_NO_BNRED" in wp.CONV_SETTINGS[name]:
                assert got["slots"] == 0, (name, r, got)
            else:
                assert got["slots"] == want, (name, r, got)
        s = table["settings"][name]
        assert name == "default" or s["conv"] or s["fold"], name
    have, have_fold = set(map(tuple, rows)), set(map(tuple, table["fold"]))
    for fn in (wp.igemm_hand_rows, wp.igemm_boundary_rows):
        conv, fold = fn()
        assert not [r for r in conv if tuple(r) not in have] and not [r for r in fold if tuple(r) not in have_fold]
    default = dict(zip(map(tuple, rows), wp.expected(table, "default")[0]))
    assert {len(a) for a in default.values()} == {1, 10}                                       # refusals and answers
    assert {r[14] for r in rows} == {0, 1, 2, 3, 4}
    assert {a[1] for a in default.values() if len(a) > 1} == {128, 256} and {a[2] for a in default.values() if len(a) > 1} == {32, 64, 128}
    assert any(r[0] * r[1] * r[2] * r[3] * 2 >= 1 << 32 for r in rows)                          # beyond the 32-bit buffer range


# ---- each *_bnred launcher needs exactly the slot count its query answers.  The slot check runs before anything is launched: with
# one slot too few the entry point refuses and names its need.  (Never slots >= the need: that would launch.)
FAKE = 4096          # never dereferenced


def _launcher_cases():
    rows, _ = wp.igemm_hand_rows()
    return sorted(set(tuple(r) for r in rows if r[14] >= 1))


@pytest.mark.parametrize("op", [1, 2, 3, 4], ids=["dgrad_bnred", "dgrad_s2_bnred", "dgrad_s2f_bnred", "dgrad_dual_bnred"])
def test_launcher_needs_the_slots_its_query_answers(built, op):
    from object_detection_cib_amd import _lib
    lib = _lib.lib()
    seen = 0
    for B, H, W, ldx, Cin, N, KH, KW, SH, SW, PH, PW, Kp, ldy, row_op in _launcher_cases():
        if row_op != op:
            continue
        if op <= 2:
            s = lib.kodhip_conv_dgrad_bnred_slots(B, H, W, Cin, N, KH, KW, SH, SW, PH, PW, ldy, op - 1)
        else:
            s = (lib.kodhip_conv_dgrad_s2f_bnred_slots if op == 3 else lib.kodhip_conv_dgrad_dual_bnred_slots)(B, H, W, Cin, N, ldy)
        if s < 2:
            continue
        seg = (_lib.KodBnRedSeg * 1)()
        seg[0].ch_begin, seg[0].ch_count, seg[0].raw, seg[0].ldr, seg[0].aff, seg[0].partials = 0, Cin, FAKE, Cin, FAKE, FAKE
        tail = (ldy, 0, 0, None, C.cast(seg, C.c_void_p), 1, s - 1, None)
        if op == 1:
            rc = lib.kodhip_conv_dgrad_bnred(FAKE, FAKE, FAKE, B, H, W, ldx, 0, Cin, N, KH, KW, SH, SW, PH, PW, Kp, *tail)
        elif op == 2:
            rc = lib.kodhip_conv_dgrad_s2_bnred(FAKE, FAKE, FAKE, B, H, W, ldx, 0, Cin, N, *tail)
        elif op == 3:
            rc = lib.kodhip_conv_dgrad_s2f_bnred(FAKE, FAKE, FAKE, B, H, W, ldx, 0, Cin, N, *tail)
        else:
            rc = lib.kodhip_conv_dgrad_dual_bnred(FAKE, FAKE, FAKE, FAKE, FAKE, B, H, W, ldx, 0, Cin, N, Kp, *tail)
        err = lib.kodhip_last_error().decode()
        m = re.search(r"partial buffers have (\d+) slots, launch needs (\d+)", err)
        assert rc < 0 and m, ((B, H, W, Cin, N), rc, err)
        assert (int(m.group(1)), int(m.group(2))) == (s - 1, s), ((B, H, W, Cin, N), s, err)
        seen += 1
    if not any(os.environ.get(k) for k in wp.CONV_KNOBS):
        assert seen >= 2, "no hand row of this form needs two slots or more"
