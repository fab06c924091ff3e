"""player.View: the zoom index and view positions Main keeps (Main.hx:170-171, 1186-1193, 1234-1278), without a GPU."""
import pytest

import view_ref as vr
from jsplayer_amd import player


def test_initial_state():
    v = player.View()
    assert (v.zoom_index, v.hor_view_pos, v.ver_view_pos) == (0, 0.5, 0.5)
    assert player.View.ZOOM_FACTORS == (0, 1, 2)


def test_zoom_saturates_at_the_ends_of_the_table():
    v = player.View()
    v.zoom_out()
    assert v.zoom_index == 0
    v.zoom_in()
    assert v.zoom_index == 1
    v.zoom_in()
    v.zoom_in()
    v.zoom_in()
    assert v.zoom_index == 2
    v.zoom_out()
    assert v.zoom_index == 1
    v.zoom_in()
    v.zoom_fit()
    assert v.zoom_index == 0
    v.zoom_fit()
    assert v.zoom_index == 0


def test_keys_are_ignored_in_fit_and_clamp_at_0_and_1():
    v = player.View()
    for code in (37, 38, 39, 40):
        v.key(code)
    assert (v.hor_view_pos, v.ver_view_pos) == (0.5, 0.5)
    v.zoom_in()
    v.key(37)
    assert v.hor_view_pos == 0.5 - 0.1 and v.ver_view_pos == 0.5
    v.key(39)
    v.key(39)
    assert v.hor_view_pos == 0.5 - 0.1 + 0.1 + 0.1
    v.key(38)
    assert v.ver_view_pos == 0.5 - 0.1
    v.key(40)
    v.key(40)
    assert v.ver_view_pos == 0.5 - 0.1 + 0.1 + 0.1
    for _ in range(12):
        v.key(37)
        v.key(38)
    assert (v.hor_view_pos, v.ver_view_pos) == (0, 0)
    for _ in range(12):
        v.key(39)
        v.key(40)
    assert (v.hor_view_pos, v.ver_view_pos) == (1, 1)
    v.key(13)                                   # any other key: nothing
    assert (v.zoom_index, v.hor_view_pos, v.ver_view_pos) == (1, 1, 1)


def test_scroll_sets_one_position():
    v = player.View()
    v.scroll(True, 0.25)
    assert (v.hor_view_pos, v.ver_view_pos) == (0.25, 0.5)
    v.scroll(False, 0.75)
    assert (v.hor_view_pos, v.ver_view_pos) == (0.25, 0.75)
    assert v.zoom_index == 0                    # (scrolling is possible in Fit: the positions wait for the next zoom)


@pytest.mark.parametrize("frame,window", [((1920, 1080), (1280, 720)), ((20, 12), (15, 9)), ((37, 23), (64, 64))])
def test_matrix_equals_the_reference(frame, window):
    v = player.View()
    for steps in range(3):
        for hor, ver in [(0.5, 0.5), (0.0, 1.0), (0.3, 0.7), (1.0, 0.0)]:
            v.scroll(True, hor)
            v.scroll(False, ver)
            assert v.matrix(*frame, *window) == vr.view_matrix(*frame, *window, player.View.ZOOM_FACTORS[v.zoom_index], hor, ver)
        v.zoom_in()
    assert v.zoom_index == 2
    assert player.View().matrix(1920, 1080, 1280, 720) == (2 / 3, 0.0, 0.0)
