"""CPU: the scene tiler against the reference's own SplitSingle (tests/golden/scene_tiles.npz, recorded by
tests/golden/make_golden_scene.py), coverage of every pixel, chip names, and the GPU-only entry points refusing
CPU tensors."""
import numpy as np
import pytest
import torch

from conftest import golden


def _cases():
    g = golden("scene_tiles.npz")
    for h, w, gap, sub, rate in g["cases"]:
        key = "g%s_h%s_w%s" % (gap, h, w)
        yield int(h), int(w), int(gap), int(sub), str(rate), g[key + "_origins"], [str(s) for s in g[key + "_names"]]


def test_fixture_holds_the_cases_the_tiler_is_pinned_on():
    cases = list(_cases())
    for gap in (200, 100):
        have = {(h, w) for h, w, g_, *_ in cases if g_ == gap}
        for e in (600, 1024, 1025, 1849, 2500, 4096):
            assert (e, e) in have
        assert sum(1 for h, w in have if h != w) >= 3
    assert {c[4] for c in cases} == {"1", "0.5", "1.5"}


def test_tile_grid_and_chip_names_equal_the_reference_splitter():
    from s2anet_amd.scene import tile_grid, chip_names
    image = str(golden("scene_tiles.npz")["image_name"])
    for h, w, gap, sub, rate, origins, names in _cases():
        got = tile_grid(h, w, sub, gap)
        assert got.dtype == np.int32 and got.shape == origins.shape, (h, w, gap)
        assert (got == origins).all(), (h, w, gap)
        r = float(rate) if "." in rate else int(rate)            # splitdata(1) / splitdata(0.5): str(rate) is the name part
        assert chip_names(image, got, r) == names, (h, w, gap)


def test_tile_grid_axis_values_of_the_loop_rules():
    from s2anet_amd.scene import tile_grid
    want = {600: [0], 1024: [0], 1025: [0, 1], 1849: [0, 824, 825], 2500: [0, 824, 1476],
            4096: [0, 824, 1648, 2472, 3072]}
    for e, axis in want.items():
        o = tile_grid(e, e)
        assert o[:: len(axis), 0].tolist() == axis and o[: len(axis), 1].tolist() == axis      # left outer, up inner
        assert o.shape[0] == len(axis) ** 2
    assert tile_grid(0, 100).shape == (0, 2)
    with pytest.raises(ValueError):
        tile_grid(100, 100, 1024, 1024)


def test_every_pixel_is_covered_and_every_tile_lies_inside():
    from s2anet_amd.scene import tile_grid
    for h, w, gap, sub, *_ in _cases():
        o = tile_grid(h, w, sub, gap)
        cover = np.zeros((h, w), bool)
        for left, up in o:
            assert 0 <= left and left + sub <= max(w, sub) and 0 <= up and up + sub <= max(h, sub), (h, w, gap, left, up)
            cover[up:up + sub, left:left + sub] = True
        assert cover.all(), (h, w, gap)
        assert len({tuple(t) for t in o.tolist()}) == len(o)                                   # no tile twice


def test_chip_names_round_trip_through_the_merge_parser():
    from s2anet_amd.merge import parse_chip_name
    from s2anet_amd.scene import tile_grid, chip_names
    for rate in (1, 0.5, 1.5):
        o = tile_grid(2500, 4096)
        for (left, up), name in zip(o.tolist(), chip_names("P0170", o, rate)):
            assert parse_chip_name(name) == ("P0170", left, up, str(rate))


def test_scene_entry_points_refuse_cpu_tensors():
    import s2anet_amd as S
    from s2anet_amd.scene import detect_scene
    scene = torch.zeros(64, 64, 3, dtype=torch.uint8)
    with pytest.raises(NotImplementedError):
        S.gather_chips(scene, S.tile_grid(64, 64, 16, 0), 16)
    with pytest.raises(NotImplementedError):
        S.merge_detections(torch.zeros(1, 4, 6), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                           np.zeros((1, 2), np.int32))
    with pytest.raises(NotImplementedError):
        detect_scene(None, scene)


def test_scene_argument_checks_return_codes_without_touching_the_gpu():
    import ctypes
    from s2anet_amd import _lib
    L = _lib.lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(1 << 20)                                      # never dereferenced
    assert L.s2a_scene_gather_u8(one, 64, 64, one, 1, 1000, one, z) == _lib.EINVAL and "multiple of 16" in L.s2a_last_error().decode()
    assert L.s2a_scene_gather_u8(one, 64, 64, one, 0, 1024, one, z) == _lib.OK
    assert L.s2a_scene_merge(one, one, one, one, z, 1, 4, 0, 0.5, 0, one, one, one, one, one, one, one, 1 << 30, z) == _lib.EINVAL
    assert L.s2a_scene_merge(one, one, one, one, z, 1, 4, 15, 0.5, 0, one, one, one, one, one, one, one, 16, z) == _lib.EWORKSPACE
    # O(rows + pairs): the default list of a 50 000-row scene stays below 2 KiB per row (a quadratic mask alone is 6 KiB)
    assert L.s2a_scene_merge_workspace_bytes(50000, 0) < 50000 * 2048
    assert L.s2a_scene_merge_workspace_bytes(625 * 2000, 0) < 625 * 2000 * 2048
