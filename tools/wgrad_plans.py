"""Weight-gradient launch plans as a table: what kodhip_conv_wgrad_plan_query, kodhip_conv_wgrad_splits_geo,
kodhip_conv_wgrad_dual_splits and kodhip_stem_bwd_fused_blocks answer for a list of layer geometries, under the default
environment and under each dispatch knob.  tests/golden/wgrad_plans.json is such a table; tests/test_wgrad_plans.py asserts
that the built library reproduces it row for row, so a change of csrc/conv_wgrad.hip's host half that moves a tile, a split
count or a slab count shows as a differing row.  The queries read no pointer and launch nothing: no GPU is needed.

A conv row is [B, H, W, ldx, Cin, N, KH, KW, SH, SW, PH, PW, Kp, ldy, dual] -> the eight plan_query outputs
{tn, tk, row3, wn, rn, wc, splits, dma} + splits_geo (dual = 0) or dual_splits (dual = 1); a stem row is [B, H, Wp, N] -> blocks.
The file keeps the default table in full and, per knob setting, only the rows whose answer differs from the default one.

usage:  python tools/wgrad_plans.py --record tests/golden/wgrad_plans.json      (every knob setting in a child process: a knob
                                                                                is read once per process)
        python tools/wgrad_plans.py --eval FILE                                 this process' answers for FILE's rows, as JSON
"""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("KODHIP_WGRAD_DMA", "KODHIP_WGRAD_ROW3", "KODHIP_WGRAD_SLOTS", "KODHIP_WGRAD_ROW3_SLOTS", "KODHIP_STEM_BWD_TW",
         "KODHIP_STEM_BWD_BLOCKS")
SETTINGS = {
    "default": {},
    "row3_off": {"KODHIP_WGRAD_ROW3": "0"},
    "row3_all": {"KODHIP_WGRAD_ROW3": "2"},
    "dma_none": {"KODHIP_WGRAD_DMA": "none"},
    "slots_256": {"KODHIP_WGRAD_SLOTS": "256"},
    "row3_slots_1536": {"KODHIP_WGRAD_ROW3_SLOTS": "1536"},
    "stem_tw_160": {"KODHIP_STEM_BWD_TW": "160"},
}
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


# ---------------------------------------------------------------------------------------------- the answers
def evaluate(conv, stem, lib_path=None):
    """-> (conv answers [9 ints per row], stem answers) of the library in THIS process' environment (plain ctypes: the
    queries need no runtime and no torch)"""
    h = C.CDLL(lib_path or os.environ.get("KODHIP_LIB") or os.path.join(ROOT, "object_detection_cib_amd", "libkodhip.so"))
    out = (C.c_int * 8)()
    ca = []
    for r in conv:
        rc = h.kodhip_conv_wgrad_plan_query(*r, out)
        assert rc == 0, (r, rc)
        B, H, W, ldx, Cin, N, KH, KW, SH, SW, PH, PW, Kp, ldy, dual = r
        slabs = h.kodhip_conv_wgrad_dual_splits(B, H, W, ldx, Cin, N, Kp, ldy) if dual else h.kodhip_conv_wgrad_splits_geo(*r[:14])
        ca.append(list(out) + [slabs])
    return ca, [h.kodhip_stem_bwd_fused_blocks(*r) for r in stem]


def run_setting(name, path):
    """the answers for the rows of `path` under knob setting `name`, from a child process"""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(SETTINGS[name])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--eval", path], capture_output=True, text=True, env=env, timeout=120)
    if r.returncode != 0:
        raise RuntimeError("wgrad_plans --eval under %s failed (rc %s):\n%s" % (name, r.returncode, r.stderr[-2000:]))
    got = json.loads(r.stdout)
    return got["conv"], got["stem"]


def conv_rows(table):
    """the file's conv rows in full: [B, H, W, ldx, Cin, N, KH, KW, SH, SW, PH, PW, Kp, ldy, dual]"""
    return [[B] + table["geo"][g] for B, g in table["conv"]]


def expected(table, name):
    """the file's answers under setting `name`: the default table with the setting's differing rows put in"""
    d, s = table["settings"]["default"], table["settings"][name]
    conv, stem = list(d["conv"]), list(d["stem"])
    if name != "default":
        for i, a in s["conv"]:
            conv[i] = a
        for i, a in s["stem"]:
            stem[i] = a
    return [table["answers"][a] for a in conv], stem


def record(path):
    """File layout (integer arrays throughout): geo = the distinct geometries without B, conv = [B, index into geo] per row,
    stem = [B, H, Wp, N] per row, answers = the distinct nine-integer answers; settings[name] = {env, conv, stem}: under
    "default" one entry per row (conv: index into answers, stem: blocks), under a knob [row, value] for the rows that differ."""
    conv, stem = all_rows()
    geo = sorted(set(tuple(r[1:]) for r in conv))
    gi = {g: i for i, g in enumerate(geo)}
    table = dict(geo=[list(g) for g in geo], conv=[[r[0], gi[tuple(r[1:])]] for r in conv], stem=stem, answers=[], settings={})
    with open(path, "w") as f:
        json.dump(table, f)
    ai, dc, ds = {}, None, None
    for name in SETTINGS:
        ca, sa = run_setting(name, path)
        ca = [ai.setdefault(tuple(a), len(ai)) for a in ca]
        if name == "default":
            dc, ds = ca, sa
            table["settings"][name] = dict(env={}, conv=ca, stem=sa)
            continue
        table["settings"][name] = dict(env=SETTINGS[name], conv=[[i, a] for i, a in enumerate(ca) if a != dc[i]],
                                       stem=[[i, a] for i, a in enumerate(sa) if a != ds[i]])
        print(name, len(table["settings"][name]["conv"]), "conv rows and", len(table["settings"][name]["stem"]),
              "stem rows differ from the default table", flush=True)
    table["answers"] = [list(a) for a in ai]
    with open(path, "w") as f:
        f.write("{\n")
        for k in ("geo", "conv", "stem", "answers"):
            f.write(' "%s": %s,\n' % (k, json.dumps(table[k], separators=(",", ":"))))
        f.write(' "settings": {\n')
        for j, (k, v) in enumerate(table["settings"].items()):
            f.write('  "%s": %s%s\n' % (k, json.dumps(v, separators=(",", ":")), "," if j + 1 < len(SETTINGS) else ""))
        f.write(" }\n}\n")
    print(len(conv), "conv rows,", len(stem), "stem rows ->", path, os.path.getsize(path), "bytes")


def main(argv):
    if len(argv) == 2 and argv[0] == "--record":
        record(argv[1])
    elif len(argv) == 2 and argv[0] == "--eval":
        table = json.load(open(argv[1]))
        ca, sa = evaluate(conv_rows(table), table["stem"])
        json.dump(dict(conv=ca, stem=sa), sys.stdout)
    else:
        print(__doc__)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
