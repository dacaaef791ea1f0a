"""CPU: the launch of mtfjsp_replay_plans (copies per workgroup, dynamic LDS bytes) as capi.replay_launch_info_for reports it equals
the rule restated in tests/replay_ref.py — at the shapes of the GPU tests, at J20M20, at the largest shapes README "Accepted shapes"
lists, and one byte below a shape's need.  No GPU: the library answers from the shape alone."""
from importlib import import_module

import pytest

import replay_ref as ref


def _capi():
    import mtfjsp_amd  # noqa: F401
    return import_module("e2e-mappo-for-mt-fjsp_amd.capi")


SHAPES = [(3, 4), (6, 6), (5, 13), (9, 15), (65, 2), (20, 20)]
LARGEST = [(36, 64), (89, 32), (186, 16)]


@pytest.mark.parametrize("batch", [1, 2, 3, 15, 32768])
@pytest.mark.parametrize("J,M", SHAPES)
def test_group_and_bytes_equal_the_model(J, M, batch):
    exp = ref.launch(J, M, batch)
    assert exp is not None
    assert _capi().replay_launch_info_for(J, M, batch) == exp
    g, nb = exp
    assert g in (1, 2, 4) and nb == g * ref.region_bytes(J, M) and nb % 16 == 0
    assert g == 1 or (nb <= ref.LDS_SOFT and g < 2 * batch)


def test_the_model_itself():
    """the numbers the rule gives where they can be worked out by hand: J6M6 is 62 bytes x 36 tasks + 288 of transport times + 31 words"""
    assert ref.region_bytes(6, 6) == 2656 and ref.launch(6, 6, 32768) == (4, 4 * 2656)
    assert ref.launch(6, 6, 1) == (1, 2656) and ref.launch(6, 6, 2) == (2, 2 * 2656) and ref.launch(6, 6, 3) == (4, 4 * 2656)
    assert ref.launch(20, 20, 4096)[0] == 2, "J20M20: 28 KB a copy, two of them within 64 KB"
    assert ref.region_bytes(9, 15) > 62 * 135 + 8 * 225


@pytest.mark.parametrize("J,M", LARGEST)
def test_the_largest_accepted_shapes_fit_or_are_refused(J, M):
    capi = _capi()
    fits = ref.fits(J, M)
    assert fits == (ref.launch(J, M, 64) is not None)
    assert not fits, "62 bytes a task: beyond T = 2 600 one copy's schedule and operands exceed a workgroup's 160 KiB"
    with pytest.raises(ValueError):
        capi.replay_launch_info_for(J, M, 64)
    # with the LDS it needs the same shape is one copy per workgroup
    need = ref.region_bytes(J, M)
    assert capi.replay_launch_info_for(J, M, 64, lds_max=need) == (1, need)


@pytest.mark.parametrize("J,M", SHAPES + LARGEST)
def test_one_byte_below_the_need_is_refused(J, M):
    capi = _capi()
    need = ref.region_bytes(J, M)
    assert capi.replay_launch_info_for(J, M, 7, lds_max=need) == ref.launch(J, M, 7, need) == (1, need)
    assert ref.launch(J, M, 7, need - 1) is None
    with pytest.raises(ValueError):
        capi.replay_launch_info_for(J, M, 7, lds_max=need - 1)


def test_shapes_the_library_refuses():
    capi = _capi()
    for J, M, batch in ((0, 4, 1), (3, 1, 1), (3, 65, 1), (3, 4, 0), (600, 64, 1)):
        with pytest.raises(ValueError):
            capi.replay_launch_info_for(J, M, batch)


def test_a_limit_between_two_and_four_copies():
    """lds_max below 64 KiB caps the soft limit too: J20M20 with room for exactly one copy, then two"""
    capi = _capi()
    nb = ref.region_bytes(20, 20)
    for lds_max, g in ((nb, 1), (2 * nb - 1, 1), (2 * nb, 2), (4 * nb, 2)):
        assert capi.replay_launch_info_for(20, 20, 100, lds_max=lds_max) == ref.launch(20, 20, 100, lds_max) == (g, g * nb)
