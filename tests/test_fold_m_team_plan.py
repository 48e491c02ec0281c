"""Host only: the slab program of the folded evaluation's M = L' P workgroups (vb_fold_m_team_plan: the function
gemm_f64_team_plan of csrc/vb_gemm_f64.h that the device code runs, and gemm_f64_team_barriers).  Two four-wave teams
share a pair of 64-row blocks: for every D the route admits up to 4096 and every pair, the two programs cover every
16-deep slab of both tiles exactly once, both teams execute the same number of barriers, and every workgroup of a shape
runs the same number of slab iterations (the middle block of an odd number of row blocks half as many)."""
import ctypes

import pytest


def _plan(lib, d, pair):
    out = (ctypes.c_int * 8)()
    from viabel_amd import _lib
    assert lib.vb_fold_m_team_plan(d, pair, out) == _lib.VB_OK
    return tuple(out)


@pytest.fixture(scope='module')
def lib():
    from viabel_amd import _lib
    return _lib.load()


def test_programs_cover_every_slab_once_with_equal_barriers(lib):
    for d in range(1024, 4097, 16):
        tiles_m = -(-d // 64)
        slabs = lambda bm: (d - 64 * bm) // 16      # noqa: E731  (the k range of a row block starts at its first row)
        iterations = set()
        for pair in range((tiles_m + 1) // 2):
            H, n_h, n_l, cnt0, cnt1, sw, bar0, bar1 = _plan(lib, d, pair)
            where = 'D=%d pair=%d' % (d, pair)
            mirror = tiles_m - 1 - pair
            assert n_h == slabs(pair) and n_l == (slabs(mirror) if mirror > pair else 0), where
            assert n_h >= 1 and 0 <= n_l <= n_h, where
            # team 0: sequence index s < sw is light slab s, beyond it heavy slab s - sw; team 1: heavy slab (H - n_l) + s
            team0 = [('light', s) if s < sw else ('heavy', s - sw) for s in range(cnt0)]
            team1 = [('heavy', H - n_l + s) for s in range(cnt1)]
            want = [('light', s) for s in range(n_l)] + [('heavy', s) for s in range(n_h)]
            assert sorted(team0 + team1) == sorted(want), where
            assert sw == n_l and cnt0 == H and cnt1 in (H, H - 1) and 0 <= cnt1, where
            if mirror > pair:
                assert 0 < sw < H, where          # the tile switch falls inside team 0's loop
                iterations.add(H)
            else:
                assert sw == 0, where             # the middle block: no light tile, the teams halve its k range
            assert bar0 == bar1 == H + 3, where
        assert len(iterations) == 1, 'D=%d' % d
        if tiles_m % 2:
            H_mid = _plan(lib, d, tiles_m // 2)[0]
            assert H_mid == (iterations.pop() + 1) // 2, 'D=%d' % d


def test_arguments_outside_the_plan_are_refused(lib):
    from viabel_amd import _lib
    out = (ctypes.c_int * 8)()
    assert lib.vb_fold_m_team_plan(1024, 8, out) == _lib.VB_ERR_INVALID       # eight pairs: 0 .. 7
    assert lib.vb_fold_m_team_plan(1040, 8, out) == _lib.VB_OK                # 17 row blocks: the middle one is pair 8
    assert lib.vb_fold_m_team_plan(1040, 9, out) == _lib.VB_ERR_INVALID
    assert lib.vb_fold_m_team_plan(1024, -1, out) == _lib.VB_ERR_INVALID
    assert lib.vb_fold_m_team_plan(1032, 0, out) == _lib.VB_ERR_INVALID       # no whole number of slabs
    assert lib.vb_fold_m_team_plan(0, 0, out) == _lib.VB_ERR_INVALID
    assert lib.vb_fold_m_team_plan(1024, 0, None) == _lib.VB_ERR_INVALID
