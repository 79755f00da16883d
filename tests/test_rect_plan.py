"""The rectangular-inference geometry and batch planner (engine/rect.py) and `inference.letterbox_table(canvas=...)` on the
CPU: the square canvas is today's letterbox, known rows, the canvas invariants, the plan's coverage, the stable order, the
pixel share of a seeded shape set, and the way back through the un-letterbox reference."""
import numpy as np
import pytest

import predict_reference as R
from object_detection_cib_amd.data.device_pipeline import VAL_DESC, letterbox_geometry
from object_detection_cib_amd.engine.rect import pixel_share, rect_batches, rect_canvas, rect_geometry, rect_order
from object_detection_cib_amd.inference import letterbox_table

# (h, w); HALVES: the short side lands on an exact .5 before rounding at S = 64 (1 x 128 -> 0.5, 3 x 128 -> 1.5, ...) or at
# S = 640 (63 x 1280 -> 31.5), where albumentations' rounding differs from Python's round()
HALVES = [(1, 128), (3, 128), (5, 128), (128, 1), (128, 7), (63, 1280), (77, 1280), (15, 128)]
SHAPES = [(720, 1280), (480, 640), (640, 480), (333, 500), (10, 1000), (640, 640), (1080, 1920), (37, 20), (171, 300), (1, 9),
          (9, 1), (64, 64), (1200, 200), (200, 1200), (641, 640), (639, 640)] + HALVES


def test_the_shape_list_holds_exact_halves():
    hit = [(h, w, S) for S in (64, 128, 640) for h, w in SHAPES
           if S != max(h, w) and abs(min(h, w) * (S / float(max(h, w))) % 1.0 - 0.5) == 0.0]
    print(f"RECT exact .5 roundings: {hit}")
    assert len(hit) >= 4


@pytest.mark.parametrize("S", [64, 128, 160, 640])
def test_square_canvas_is_letterbox_geometry(S):
    for h, w in SHAPES:
        assert rect_geometry(h, w, S, S, S) == letterbox_geometry(h, w, S), (h, w, S)


def test_known_rows_at_640():
    want = {(720, 1280): (384, 640), (480, 640): (480, 640), (333, 500): (448, 640), (10, 1000): (64, 640), (640, 640): (640, 640),
            (640, 480): (640, 480), (1080, 1920): (384, 640)}
    for shp, canvas in want.items():
        assert rect_canvas([shp], 640) == canvas, shp
    assert rect_geometry(720, 1280, 640, 384, 640) == (360, 640, 12, 0)
    assert rect_geometry(480, 640, 640, 480, 640) == (480, 640, 0, 0)
    assert rect_geometry(333, 500, 640, 448, 640) == (426, 640, 11, 0)
    assert rect_geometry(10, 1000, 640, 64, 640) == (6, 640, 29, 0)
    # several members: the canvas of the largest sides
    assert rect_canvas([(720, 1280), (480, 640), (100, 300)], 640) == (480, 640)
    assert rect_canvas([(640, 480), (480, 640)], 640) == (640, 640)


def test_canvas_invariants():
    rng = np.random.default_rng(1)
    for S in (64, 160, 640):
        for _ in range(200):
            shapes = [tuple(int(v) for v in rng.integers(1, 1500, 2)) for _ in range(int(rng.integers(1, 6)))]
            H, W = rect_canvas(shapes, S)
            assert H % 32 == 0 and W % 32 == 0 and min(S, 64) <= H <= S and min(S, 64) <= W <= S
            for h, w in shapes:
                nh, nw, top, left = rect_geometry(h, w, S, H, W)
                assert (nh, nw) == letterbox_geometry(h, w, S)[:2]
                assert 0 <= top and top + nh <= H and 0 <= left and left + nw <= W
                assert top == (H - nh) // 2 and left == (W - nw) // 2
    with pytest.raises(ValueError):
        rect_canvas([], 640)
    with pytest.raises(ValueError):
        rect_canvas([(0, 5)], 640)
    with pytest.raises(ValueError):
        rect_canvas([(5, 5)], 100)


@pytest.mark.parametrize("sort", [True, False])
def test_batches_cover_every_index_once(sort):
    rng = np.random.default_rng(2)
    for n, B in ((0, 4), (1, 4), (10, 4), (16, 16), (33, 16), (7, 1)):
        shapes = rng.integers(20, 900, (n, 2)).tolist()
        plan = rect_batches(shapes, 640, B, sort=sort)
        idx = [k for part, _, _ in plan for k in part]
        assert sorted(idx) == list(range(n)) and all(1 <= len(part) <= B for part, _, _ in plan)
        assert len(plan) == -(-n // B)
        assert idx == (rect_order(shapes).tolist() if sort else list(range(n)))
        for part, H, W in plan:
            assert (H, W) == rect_canvas([shapes[k] for k in part], 640)
    with pytest.raises(ValueError):
        rect_batches([(5, 5)], 640, 0)


def test_order_is_stable_under_ties():
    shapes = [(480, 640), (100, 100), (240, 320), (50, 50), (3, 4), (640, 480), (200, 200), (6, 8)]
    assert rect_order(shapes).tolist() == [0, 2, 4, 7, 1, 3, 6, 5]
    ratios = [h / w for h, w in shapes]
    assert all(ratios[a] <= ratios[b] for a, b in zip(rect_order(shapes)[:-1], rect_order(shapes)[1:]))
    assert rect_order([]).tolist() == []


def test_pixel_share_of_the_seeded_set():
    shapes = np.random.default_rng(0).integers(200, 1201, (5000, 2)).tolist()
    sorted_plan, plain_plan = rect_batches(shapes, 640, 16), rect_batches(shapes, 640, 16, sort=False)
    a, b = pixel_share(sorted_plan, 640), pixel_share(plain_plan, 640)
    print(f"RECT pixel share: sorted {a:.4f} ({len({(H, W) for _, H, W in sorted_plan})} canvases), unsorted {b:.4f}")
    assert a < 0.70 and b > 0.95


def test_table_on_a_canvas_and_back_to_image_pixels():
    S = 640
    shapes = [(720, 1280), (333, 500), (480, 640), (37, 20), (1080, 1920), (171, 300)]
    # canvas None is today's table
    d0, b0 = letterbox_table(shapes, S)
    for (h, w), d, b in zip(shapes, d0, b0):
        nh, nw, top, left = letterbox_geometry(h, w, S)
        assert (d["nh"], d["nw"], d["top"], d["left"]) == (nh, nw, top, left)
        assert b.tolist() == [left, top, np.float32(w / nw), np.float32(h / nh), w, h]
    sq = letterbox_table(shapes, S, canvas=(S, S))
    assert sq[0].tobytes() == d0.tobytes() and sq[1].tobytes() == b0.tobytes()
    H, W = rect_canvas(shapes, S)
    assert (H, W) == (640, 640)                                     # (37 x 20 is upright)
    for part in (shapes[:3], shapes[3:4], shapes[4:]):
        H, W = rect_canvas(part, S)
        descs, boxes = letterbox_table(part, S, canvas=(H, W))
        for (h, w), d, lb in zip(part, descs, boxes):
            nh, nw, top, left = rect_geometry(h, w, S, H, W)
            assert (d["h"], d["w"], d["nh"], d["nw"], d["top"], d["left"]) == (h, w, nh, nw, top, left)
            assert (d["scale_x"], d["scale_y"]) == (1.0 / (nw / float(w)), 1.0 / (nh / float(h)))
            assert lb.tolist() == [left, top, np.float32(w / nw), np.float32(h / nh), w, h]
            # image corners and inner points -> canvas (as DeviceValPipeline moves targets) -> back
            pts = np.array([[0, 0, w, h], [w / 3.0, h / 3.0, w / 2.0, h / 2.0], [1, 1, w - 1, h - 1]], dtype=np.float64)
            on = pts.copy()
            on[:, [0, 2]] = on[:, [0, 2]] / w * nw + left
            on[:, [1, 3]] = on[:, [1, 3]] / h * nh + top
            assert on[:, [0, 2]].min() >= left and on[:, [0, 2]].max() <= left + nw <= W
            assert on[:, [1, 3]].min() >= top and on[:, [1, 3]].max() <= top + nh <= H
            rows = np.concatenate((on, np.ones((len(on), 2))), axis=1).astype(np.float32)
            back = R.unletterbox_ref(rows, lb)[:, :4]
            # three fp32 roundings on the way (the canvas coordinate, the difference, the product by fp32(w / nw)), the
            # first two magnified by the scale: within 4 ulps of the image's longest side
            tol = 4 * np.spacing(np.float32(max(h, w)))
            assert np.abs(back - pts).max() <= tol, (h, w, np.abs(back - pts).max(), tol)
    with pytest.raises(ValueError, match="image 3"):
        letterbox_table([(640, 480)], S, first_index=3, canvas=(384, 640))


def test_the_three_geometry_names_are_one_function():
    """`letterbox_geometry` (data/device_pipeline.py), `rect_geometry` on the square (engine/rect.py) and
    `tiles._letterbox_geometry` (engine/tiles.py) answer alike on a seeded set of shapes and on the exact halves"""
    from object_detection_cib_amd.engine import tiles
    rng = np.random.default_rng(11)
    cases = [(int(h), int(w), S) for S in (64, 128, 640) for h, w in rng.integers(1, 2000, (120, 2))]
    cases += [(h, w, S) for S in (64, 128, 640) for h, w in SHAPES]
    assert len(cases) >= 400
    for h, w, S in cases:
        g = letterbox_geometry(h, w, S)
        assert g == rect_geometry(h, w, S, S, S) == tiles._letterbox_geometry(h, w, S), (h, w, S)
        assert all(type(v) is int for v in g)


@pytest.mark.parametrize("canvas", [None, (384, 640)])
def test_letterbox_table_records_are_the_geometry_field_by_field(canvas):
    """what DeviceValPipeline.make_batch uploads (`letterbox_table`'s records plus the pool offsets): every field against
    values formed here from the geometry, the two scales as OpenCV forms them (1 / inv_scale, in double)"""
    S = 640
    shapes = [(720, 1280), (360, 640), (63, 1280), (100, 300), (384, 640), (1, 9)]
    descs, rows = letterbox_table(shapes, S, canvas=canvas)
    assert descs.dtype == VAL_DESC and len(descs) == len(shapes) and not descs["off"].any()
    for d, row, (h, w) in zip(descs, rows, shapes):
        nh, nw, top, left = letterbox_geometry(h, w, S) if canvas is None else rect_geometry(h, w, S, *canvas)
        assert (int(d["h"]), int(d["w"]), int(d["nh"]), int(d["nw"]), int(d["top"]), int(d["left"])) == (h, w, nh, nw, top, left)
        assert float(d["scale_x"]) == 1.0 / (nw / float(w)) and float(d["scale_y"]) == 1.0 / (nh / float(h))
        assert row.tolist() == [left, top, np.float32(w / float(nw)), np.float32(h / float(nh)), w, h]
    # a sequence as first_index names each image by its own number (make_batch: the pool index)
    with pytest.raises(ValueError, match="image 41: "):
        letterbox_table([(360, 640), (1, 2000)], S, [40, 41], canvas)
