"""Weight-gradient launch plans as a table: what kodhip_conv_wgrad_plan_query, kodhip_conv_wgrad_splits_geo,
kodhip_conv_wgrad_dual_splits and kodhip_stem_bwd_fused_blocks answer for a list of layer geometries, under the default
environment and under each dispatch knob.  tests/golden/wgrad_plans.json is such a table; tests/test_wgrad_plans.py asserts
that the built library reproduces it row for row, so a change of csrc/conv_wgrad.hip's host half that moves a tile, a split
count or a slab count shows as a differing row.  The queries read no pointer and launch nothing: no GPU is needed.

A conv row is [B, H, W, ldx, Cin, N, KH, KW, SH, SW, PH, PW, Kp, ldy, dual] -> the eight plan_query outputs
{tn, tk, row3, wn, rn, wc, splits, dma} + splits_geo (dual = 0) or dual_splits (dual = 1); a stem row is [B, H, Wp, N] -> blocks.
The file keeps the default table in full and, per knob setting, only the rows whose answer differs from the default one.

The same machinery records csrc/conv_igemm.hip's plans (forward, data gradients): tests/golden/conv_plans.json.gz, asserted by
tests/test_conv_plans.py.  There a conv row is [B, H, W, ldx, Cin, N, KH, KW, SH, SW, PH, PW, Kp, ldy, op] (op as
kodhip_conv_plan_query takes it, channel offsets 0) -> [0, the eight plan_query outputs {bm, bn, row3, fast, tiles_m, tiles_n,
groups_m, merged}, the op's slot query], or [return code] alone where the query refuses; the second list ("fold" in place of
"stem") is [Cin, N] -> kodhip_conv_dgrad_s2_folded.  The file says which table it holds ("table": "conv"; none = this one).
A file whose name ends in .gz is the same JSON text gzip-compressed (the conv table is 290 KB of integers as text, 60 KB so).

usage:  python tools/wgrad_plans.py --record tests/golden/wgrad_plans.json      (every knob setting in a child process: a knob
                                                                                is read once per process)
        python tools/wgrad_plans.py --record-conv tests/golden/conv_plans.json.gz
        python tools/wgrad_plans.py --eval FILE                                 this process' answers for FILE's rows, as JSON
"""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("KODHIP_WGRAD_DMA", "KODHIP_WGRAD_ROW3", "KODHIP_WGRAD_SLOTS", "KODHIP_WGRAD_ROW3_SLOTS", "KODHIP_STEM_BWD_BLOCKS")
SETTINGS = {
    "default": {},
    "row3_off": {"KODHIP_WGRAD_ROW3": "0"},
    "row3_all": {"KODHIP_WGRAD_ROW3": "2"},
    "dma_none": {"KODHIP_WGRAD_DMA": "none"},
    "slots_256": {"KODHIP_WGRAD_SLOTS": "256"},
    "row3_slots_1536": {"KODHIP_WGRAD_ROW3_SLOTS": "1536"},
}
CONV_KNOBS = ("KODHIP_FORCE_BN", "KODHIP_FORCE_BM", "KODHIP_ROW3", "KODHIP_NO_FAST", "KODHIP_S2_SEPARATE", "KODHIP_S2_FOLD_MAXC",
              "KODHIP_NO_BNRED")
CONV_SETTINGS = {
    "default": {},
    "row3_off": {"KODHIP_ROW3": "0"},
    "row3_128": {"KODHIP_ROW3": "1"},
    "no_fast": {"KODHIP_NO_FAST": "1"},
    "force_bn_32": {"KODHIP_FORCE_BN": "32"},
    "force_bn_64": {"KODHIP_FORCE_BN": "64"},
    "force_bn_128": {"KODHIP_FORCE_BN": "128"},
    "force_bm_128": {"KODHIP_FORCE_BM": "128"},
    "force_bm_256": {"KODHIP_FORCE_BM": "256"},
    "s2_separate": {"KODHIP_S2_SEPARATE": "1"},
    "no_bnred": {"KODHIP_NO_BNRED": "1"},
    "s2_fold_never": {"KODHIP_S2_FOLD_MAXC": "0"},
}
# per table: (knob settings, key of the file's second row list)
TABLES = {"wgrad": (SETTINGS, "stem"), "conv": (CONV_SETTINGS, "fold")}
pad = lambda v, m: (v + m - 1) // m * m


# ---------------------------------------------------------------------------------------------- the rows
def network_rows():
    """every conv unit, dual pair, head and the stem of yv5n / yv5s / yv5m at 64, 160, 416, 640 px for B = 1, 16, 64"""
    sys.path.insert(0, ROOT)
    from object_detection_cib_amd.engine.graph import build_graph
    conv, stem = [], []
    npad = pad(3 * (5 + 10), 8)
    for widen, deepen in ((0.25, 0.33), (0.5, 0.33), (0.75, 0.67)):
        g = build_graph(3, 10, widen, deepen)
        for S in (64, 160, 416, 640):
            for B in (1, 16, 64):
                for u in g.units:
                    if u.stem:
                        conv.append([B, S, S // 2, 8, 8, u.cout, 6, 3, 2, 1, 2, 1, 160, u.cout, 0])
                        stem.append([B, S, S // 2, u.cout])
                        continue
                    H = S // u.src.stride
                    Kp = pad(u.k * u.k * u.cin, 32)
                    conv.append([B, H, H, u.src.buf.C, u.cin, u.cout, u.k, u.k, u.s, u.s, u.p, u.p, Kp, u.cout, 0])
                    if u.sibling is not None and u.k == 1 and u.s == 1:
                        conv.append([B, H, H, u.src.buf.C, u.cin, u.cout, 1, 1, 1, 1, 0, 0, Kp, u.cout, 1])
                for h in g.heads:
                    H = S // h.stride
                    conv.append([B, H, H, h.src.buf.C, h.cin, npad, 1, 1, 1, 1, 0, 0, pad(h.cin, 32), npad, 0])
    return conv, stem


def hand_rows():
    """the hand cases of tests/test_hip_conv_exact.py and tests/test_abi.py"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import test_hip_conv_exact as t

    def sq(B, Cin, H, W, N, k, s, p, dual=0, ldx=None):
        return [B, H, W, ldx or Cin, Cin, N, k, k, s, s, p, p, pad(k * k * Cin, 32), N, dual]
    rows = [sq(*c[:8]) for c in t.CASES.values() if "w" in c[8]]
    rows += [sq(*geo) for geo, _ in t.WGRAD_CFG]
    rows += [sq(2, cn[0], 20, 12, cn[1], 3, 1, 1) for cn, _ in t.WGRAD_ROW3]
    for (B, Cin, H, W, N), _ in t.WGRAD_DUAL:
        rows += [sq(B, Cin, H, W, N, 1, 1, 0, dual=1, ldx=Cin + 16), sq(B, Cin, H, W, N, 1, 1, 0, dual=1)]
    stem = []
    for N, B, H, W, _ in t.STEM_CASES:
        rows.append([B, H, W // 2, 8, 8, N, 6, 3, 2, 1, 2, 1, 160, N, 0])
        stem.append([B, H, W // 2, N])
    # tests/test_abi.py::test_plan_queries_launch_nothing
    rows += [sq(2, 32, 20, 12, 32, 3, 1, 1), sq(2, 64, 20, 12, 64, 3, 1, 1), sq(2, 32, 20, 12, 32, 3, 2, 1),
             sq(2, 64, 70, 65, 32, 1, 1, 0), sq(2, 64, 70, 65, 32, 1, 1, 0, dual=1)]
    return rows, stem


def boundary_rows():
    """N and Kp at every boundary of the tile rule, both forms; the ROW3 rule's boundaries; operands beyond the 32-bit buffer
    range (nothing is allocated: the queries read no pointer)"""
    rows = []
    for N in (8, 32, 33, 64, 65, 128, 129, 192, 193, 256):
        for Kp in (32, 64, 128, 160, 288):
            for dual in (0, 1):
                rows.append([2, 70, 65, Kp, Kp, N, 1, 1, 1, 1, 0, 0, Kp, pad(N, 8), dual])
            rows.append([16, 40, 40, Kp, Kp, N, 1, 1, 1, 1, 0, 0, Kp, pad(N, 8), 0])
    for Cin in (32, 48, 64, 224, 256, 288):
        for N in (8, 32, 40, 64, 72, 128, 256, 264):
            for B, H in ((2, 20), (64, 80)):
                rows.append([B, H, H, Cin, Cin, N, 3, 3, 1, 1, 1, 1, pad(9 * Cin, 32), N, 0])
    for Cin, N, k, p in ((64, 32, 1, 0), (32, 32, 3, 1), (256, 256, 3, 1), (64, 64, 1, 0)):
        Kp = pad(k * k * Cin, 32)
        for ldx, ldy in ((512, N), (Cin, 512), (512, 512)):
            rows.append([64, 320, 320, ldx, Cin, N, k, k, 1, 1, p, p, Kp, ldy, 0])
            if k == 1:
                rows.append([64, 320, 320, ldx, Cin, N, 1, 1, 1, 1, 0, 0, Kp, ldy, 1])
    stem = [[B, H, Wp, N] for N in (16, 32, 48, 64) for Wp in (32, 80, 160, 320) for B, H in ((1, 2 * Wp), (64, 2 * Wp))]
    return rows, stem


def all_rows():
    conv, stem = [], []
    for fn in (network_rows, hand_rows, boundary_rows):
        c, s = fn()
        conv += c
        stem += s
    uniq = lambda rows: [list(r) for r in sorted(set(map(tuple, rows)))]
    return uniq(conv), uniq(stem)


# ------------------------------------------------------------------ the rows, read for csrc/conv_igemm.hip's entry points
def igemm_rows(conv):
    """the rows above as kodhip_conv_plan_query takes them.  A row above names the forward layer; each entry point has its own Kp
    = taps x round_up(channels per tap, 32): the forward's per Cin, the data gradient's per N.  -> (conv rows, fold rows)"""
    rows, fold = [], []
    for B, H, W, ldx, Cin, N, KH, KW, SH, SW, PH, PW, _, ldy, dual in conv:
        if (ldx, Cin, KH, KW) == (8, 8, 6, 3):                     # the stem: op 0 in its wide-pixel form
            rows.append([B, H, W, 8, 32, N, 6, 1, 2, 1, 2, 1, 192, ldy, 0])
        elif dual:
            rows.append([B, H, W, ldx, Cin, N, 1, 1, 1, 1, 0, 0, pad(N, 32), ldy, 4])
        else:
            geo = [KH, KW, SH, SW, PH, PW]
            rows.append([B, H, W, ldx, Cin, N] + geo + [KH * KW * pad(Cin, 32), ldy, 0])
            rows.append([B, H, W, ldx, Cin, N] + geo + [KH * KW * pad(N, 32), ldy, 1])
            if geo == [3, 3, 2, 2, 1, 1] and H % 2 == 0 and W % 2 == 0:
                rows += [[B, H, W, ldx, Cin, N] + geo + [0, ldy, 2], [B, H, W, ldx, Cin, N] + geo + [0, ldy, 3]]
                fold.append([Cin, N])
    return rows, fold


def igemm_hand_rows():
    """the hand cases of tests/test_hip_conv_exact.py (with the ops each names), the geometries of tests/test_hip_conv_fused.py
    and the conv half of tests/test_abi.py::test_plan_queries_launch_nothing"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import fused_reference as fr
    import test_hip_conv_exact as t

    def q(op, B, Cin, H, W, N, k, s, p):
        Kp = {0: k * k * pad(Cin, 32), 1: k * k * pad(N, 32), 2: 0, 3: 0, 4: pad(N, 32)}[op]
        return [B, H, W, Cin, Cin, N, k, k, s, s, p, p, Kp, N, op]
    rows = []
    for c in list(t.CASES.values()) + list(t.CASES_ROW3_OFF.values()):
        rows += [q("fdco".index(o), *c[:8]) for o in c[8] if o in "fdco"]
    rows += [q(0, *c[0]) for c in fr.CASES.values()]
    for N, B, H, W, _ in list(t.STEM_CASES) + list(fr.STEM_CASES):
        rows.append([B, H, W // 2, 8, 32, N, 6, 1, 2, 1, 2, 1, 192, N, 0])
    rows += [q(0, 1, 512, 128, 128, 64, 1, 1, 0), q(0, 1, 512, 127, 128, 64, 1, 1, 0), q(0, 1, 480, 128, 128, 64, 1, 1, 0),
             q(0, 1, 512, 128, 128, 32, 1, 1, 0), q(0, 5, 64, 60, 56, 160, 3, 1, 1), q(2, 4, 64, 128, 128, 128, 3, 2, 1),
             q(1, 4, 64, 128, 128, 128, 3, 2, 1), q(3, 2, 32, 16, 16, 64, 3, 2, 1), q(0, 1, 32, 130, 128, 512, 3, 1, 1)]
    conv, fold = igemm_rows(hand_rows()[0])
    return rows + conv, fold


def igemm_boundary_rows():
    """M on both sides of 256 * 64, K on both sides of 512 and N at every boundary of the tile rule, as pointwise and 3x3 layers in
    ops 0 and 1 and as stride-2 layers in ops 2 and 3; the dual form over the same N; the rows above (beyond the 32-bit buffer
    range among them)"""
    rows, fold = igemm_rows(boundary_rows()[0])
    widths = (32, 33, 40, 64, 65, 72, 96, 128, 129, 136, 192, 256)
    for H in (127, 128):                                        # M = 16256 | 16384
        for K in (480, 512):
            for N in widths:
                rows += [[1, H, 128, K, K, N, 1, 1, 1, 1, 0, 0, K, pad(N, 8), 0],
                         [1, H, 128, pad(N, 8), N, K, 1, 1, 1, 1, 0, 0, K, K, 1],
                         [1, H, 128, pad(N, 8), N, K // 2, 1, 1, 1, 1, 0, 0, pad(K // 2, 32), K // 2, 4]]
    for H in (126, 128):
        for C in (32, 64):                                      # K = 288 | 576
            for N in widths:
                rows += [[1, H, 128, C, C, N, 3, 3, 1, 1, 1, 1, 9 * C, pad(N, 8), 0],
                         [1, H, 128, pad(N, 8), N, C, 3, 3, 1, 1, 1, 1, 9 * C, C, 1]]
                s2 = [2 * H, 256, pad(N, 8), N, C, 3, 3, 2, 2, 1, 1]
                rows += [[1] + s2 + [0, C, 2], [1] + s2 + [0, C, 3]]
                fold.append([N, C])
    return rows, fold


def all_igemm_rows():
    conv, fold = [], []
    for fn in (lambda: igemm_rows(network_rows()[0]), igemm_hand_rows, igemm_boundary_rows):
        c, f = fn()
        conv += c
        fold += f
    fold += [[c, 64] for c in (8, 56, 64, 72, 128)]            # the fold threshold
    uniq = lambda rows: [list(r) for r in sorted(set(map(tuple, rows)))]
    return uniq(conv), uniq(fold)


# ---------------------------------------------------------------------------------------------- the answers
def load(lib_path=None):
    return C.CDLL(lib_path or os.environ.get("KODHIP_LIB") or os.path.join(ROOT, "object_detection_cib_amd", "libkodhip.so"))


def evaluate_igemm(conv, fold, lib_path=None):
    """-> (conv answers: [0, the eight outputs, slots] or [rc], fold answers) of the library in THIS process' environment"""
    h = load(lib_path)
    h.kodhip_conv_stats_slots.argtypes = [C.c_long, C.c_int]
    out = (C.c_int * 8)()
    ca = []
    for B, H, W, ldx, Cin, N, KH, KW, SH, SW, PH, PW, Kp, ldy, op in conv:
        rc = h.kodhip_conv_plan_query(op, B, H, W, ldx, 0, Cin, N, KH, KW, SH, SW, PH, PW, Kp, ldy, 0, out)
        if rc != 0:
            ca.append([rc])
            continue
        if op == 0:
            kw = Cin // ldx - 1 if Cin > ldx and KW == 1 else KW          # the stem's window ends in a padding pixel
            slots = h.kodhip_conv_stats_slots(B * ((H + 2 * PH - KH) // SH + 1) * ((W + 2 * PW - kw) // SW + 1), N)
        elif op <= 2:
            slots = h.kodhip_conv_dgrad_bnred_slots(B, H, W, Cin, N, KH, KW, SH, SW, PH, PW, ldy, op - 1)
        else:
            slots = (h.kodhip_conv_dgrad_s2f_bnred_slots if op == 3 else h.kodhip_conv_dgrad_dual_bnred_slots)(B, H, W, Cin, N, ldy)
        ca.append([0] + list(out) + [slots])
    return ca, [h.kodhip_conv_dgrad_s2_folded(*r) for r in fold]


def evaluate(conv, stem, lib_path=None):
    """-> (conv answers [9 ints per row], stem answers) of the library in THIS process' environment (plain ctypes: the
    queries need no runtime and no torch)"""
    h = load(lib_path)
    out = (C.c_int * 8)()
    ca = []
    for r in conv:
        rc = h.kodhip_conv_wgrad_plan_query(*r, out)
        assert rc == 0, (r, rc)
        B, H, W, ldx, Cin, N, KH, KW, SH, SW, PH, PW, Kp, ldy, dual = r
        slabs = h.kodhip_conv_wgrad_dual_splits(B, H, W, ldx, Cin, N, Kp, ldy) if dual else h.kodhip_conv_wgrad_splits_geo(*r[:14])
        ca.append(list(out) + [slabs])
    return ca, [h.kodhip_stem_bwd_fused_blocks(*r) for r in stem]


def load_table(path):
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path)) as f:
        return json.load(f)


def write_table(path, text):
    if path.endswith(".gz"):
        with open(path, "wb") as f, gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as z:       # (no name, no time: same bytes each run)
            z.write(text.encode())
    else:
        with open(path, "w") as f:
            f.write(text)


def kind(table):
    return table.get("table", "wgrad")


def run_setting(name, path):
    """the answers for the rows of `path` under knob setting `name` of the file's table, from a child process"""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS + CONV_KNOBS}
    env.update(TABLES[kind(load_table(path))][0][name])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--eval", path], capture_output=True, text=True, env=env, timeout=120)
    if r.returncode != 0:
        raise RuntimeError("wgrad_plans --eval under %s failed (rc %s):\n%s" % (name, r.returncode, r.stderr[-2000:]))
    got = json.loads(r.stdout)
    return got["conv"], got["aux"]


def conv_rows(table):
    """the file's conv rows in full: [B, H, W, ldx, Cin, N, KH, KW, SH, SW, PH, PW, Kp, ldy, dual]"""
    return [[B] + table["geo"][g] for B, g in table["conv"]]


def expected(table, name):
    """the file's answers under setting `name`: the default table with the setting's differing rows put in"""
    d, s, aux = table["settings"]["default"], table["settings"][name], TABLES[kind(table)][1]
    conv, stem = list(d["conv"]), list(d[aux])
    if name != "default":
        for i, a in s["conv"]:
            conv[i] = a
        for i, a in s[aux]:
            stem[i] = a
    return [table["answers"][a] for a in conv], stem


def record(path, which="wgrad"):
    """File layout (integer arrays throughout): geo = the distinct geometries without B, conv = [B, index into geo] per row,
    stem = [B, H, Wp, N] per row, answers = the distinct nine-integer answers; settings[name] = {env, conv, stem}: under
    "default" one entry per row (conv: index into answers, stem: blocks), under a knob [row, value] for the rows that differ.
    (The conv table: "table": "conv", "fold" = [Cin, N] per row in place of "stem".)"""
    SETTINGS, aux = TABLES[which]
    conv, stem = all_rows() if which == "wgrad" else all_igemm_rows()
    geo = sorted(set(tuple(r[1:]) for r in conv))
    gi = {g: i for i, g in enumerate(geo)}
    table = dict(geo=[list(g) for g in geo], conv=[[r[0], gi[tuple(r[1:])]] for r in conv], answers=[], settings={})
    table[aux] = stem
    if which != "wgrad":
        table["table"] = which
    write_table(path, json.dumps(table))
    ai, dc, ds = {}, None, None
    for name in SETTINGS:
        ca, sa = run_setting(name, path)
        ca = [ai.setdefault(tuple(a), len(ai)) for a in ca]
        if name == "default":
            dc, ds = ca, sa
            table["settings"][name] = {"env": {}, "conv": ca, aux: sa}
            continue
        table["settings"][name] = {"env": SETTINGS[name], "conv": [[i, a] for i, a in enumerate(ca) if a != dc[i]],
                                   aux: [[i, a] for i, a in enumerate(sa) if a != ds[i]]}
        print(name, len(table["settings"][name]["conv"]), "conv rows and", len(table["settings"][name][aux]),
              aux, "rows differ from the default table", flush=True)
    table["answers"] = [list(a) for a in ai]
    text = "{\n"
    for k in ("table", "geo", "conv", aux, "answers"):
        if k in table:
            text += ' "%s": %s,\n' % (k, json.dumps(table[k], separators=(",", ":")))
    text += ' "settings": {\n'
    for j, (k, v) in enumerate(table["settings"].items()):
        text += '  "%s": %s%s\n' % (k, json.dumps(v, separators=(",", ":")), "," if j + 1 < len(SETTINGS) else "")
    write_table(path, text + " }\n}\n")
    print(len(conv), "conv rows,", len(stem), aux, "rows ->", path, os.path.getsize(path), "bytes")


def main(argv):
    if len(argv) == 2 and argv[0] in ("--record", "--record-conv"):
        record(argv[1], "wgrad" if argv[0] == "--record" else "conv")
    elif len(argv) == 2 and argv[0] == "--eval":
        table = load_table(argv[1])
        ca, sa = (evaluate if kind(table) == "wgrad" else evaluate_igemm)(conv_rows(table), table[TABLES[kind(table)][1]])
        json.dump(dict(conv=ca, aux=sa), sys.stdout)
    else:
        print(__doc__)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
