"""A filtered film in a render sharded by tiles, host side (include/ppg.h "Footprint hook"): the number of border slots the ranks exchange
equals a brute-force count, and check_shardable lets a filtered scene through only for a reducer that exchanges footprints."""
import numpy as np
import pytest


def _brute_force_slots(W, H, tile, world, B):
    """Border slots straight from the definition: (source pixel, tap) whose target lies in the film on a tile of another rank."""
    tiles_x = -(-W // tile)
    y, x = np.mgrid[0:H, 0:W]
    owner = ((y // tile) * tiles_x + x // tile) % world
    m = 0
    for dy in range(-B, B + 1):
        for dx in range(-B, B + 1):
            ty, tx = y + dy, x + dx
            inside = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
            m += int((inside & (owner[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)] != owner)).sum())
    return m


@pytest.mark.parametrize("film", [(20, 12), (40, 28)], ids=lambda f: "%dx%d" % f)
def test_halo_floats_equal_a_brute_force_count(hip_lib_path, film):
    from ppg_host.bindings import footprint_halo_floats
    W, H = film
    nonzero = 0
    for tile in (4, 8, 16):
        for world in (1, 2, 3):
            for B in (1, 2, 3):
                got = footprint_halo_floats(W, H, tile, world, B)
                assert got == 7 * _brute_force_slots(W, H, tile, world, B), (tile, world, B)
                assert (got == 0) == (world == 1 or -(-W // tile) * -(-H // tile) == 1), (tile, world, B)
                nonzero += got > 0
    assert nonzero >= 12


def test_halo_floats_edge_cases(hip_lib_path):
    from ppg_host.bindings import footprint_halo_floats
    # 40 x 28 in tiles of 4: 10 tiles per row, a multiple of world = 2 — every tile column belongs to one rank, only left / right neighbours cross
    W, H, tile, world = 40, 28, 4, 2
    for B in (1, 2, 3):
        got = footprint_halo_floats(W, H, tile, world, B)
        assert got == 7 * _brute_force_slots(W, H, tile, world, B)
        # taps with dx = 0 never cross; a tap (dx, dy) crosses where x and x + dx lie in tile columns of different parity
        cross = sum(sum(1 for x in range(W) if 0 <= x + dx < W and (x // tile + (x + dx) // tile) % 2) * (H - abs(dy))
                    for dy in range(-B, B + 1) for dx in range(-B, B + 1))
        assert got == 7 * cross
    # the default box keeps its own-pixel film (no footprint: border 0), one rank exchanges nothing, nonsense gives 0
    assert footprint_halo_floats(40, 28, 8, 2, 0) == 0
    assert footprint_halo_floats(40, 28, 8, 1, 2) == 0
    assert footprint_halo_floats(0, 28, 8, 2, 2) == 0 and footprint_halo_floats(40, 28, 0, 2, 2) == 0
    # one tile covers the film: nothing crosses
    assert footprint_halo_floats(20, 12, 32, 3, 3) == 0


def test_check_shardable_wants_a_reducer_that_exchanges_footprints():
    from ppg_host.distributed import HostReducer, StagedReducer, TorchReducer, check_shardable
    from ppg_host.scenes import cbox_scene
    s = cbox_scene(8, 8)
    torch_red, staged, host = (object.__new__(c) for c in (TorchReducer, StagedReducer, HostReducer))  # (no process group needed to ask)
    for red in (None, torch_red, staged, host):
        check_shardable(s, red)  # the default box: any reducer
    s.rfilter = {"type": "gaussian"}
    with pytest.raises(ValueError, match="sharded filtered renders are not supported yet"):
        check_shardable(s)
    with pytest.raises(ValueError, match="sharded filtered renders are not supported yet"):
        check_shardable(s, host)  # the oracle has no film filter
    check_shardable(s, torch_red)
    check_shardable(s, staged)


def test_reducer_install_sets_the_footprint_hook():
    from ppg_host.distributed import HostReducer, TorchReducer

    class FakeEngine:
        hook = "unset"

        def set_footprint_hook(self, fn):
            self.hook = fn
    red, e = object.__new__(TorchReducer), FakeEngine()
    red.install(e)
    assert e.hook == red.reduce_footprint
    host, o = object.__new__(HostReducer), FakeEngine()
    host.install(o)
    assert o.hook == "unset"
