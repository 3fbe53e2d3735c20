"""The LDS image of the rotated conv mode's extended frame tile, on paper (tools/conv_rotate_lds_image.py): conflict-free for every
start row, a bijection for the LDS-DMA, and the control (today's blocked reads on the blocked image) conflict-free as measured."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("conv_rotate_lds_image", os.path.join(ROOT, "tools", "conv_rotate_lds_image.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_rotated_image_is_conflict_free_and_complete():
    t = _tool()
    res = t.report()
    assert res["rotated reads, rotated image"] == 1
    assert res["blocked reads, blocked image (control)"] == 1
    assert res["rotated reads, blocked image"] > 1            # why the image had to change
    assert t.rotated_image_is_bijection()


def test_tool_and_kernel_agree_on_the_plane_height():
    t = _tool()
    with open(os.path.join(ROOT, "wfl-asr_amd", "csrc", "gemm_stream.hip")) as f:
        src = f.read()
    assert f"#define XROT_ROWS {t.XROT_ROWS}\n" in src
    # the farthest row a wave reads: second wave group (96) + 31 (tap 32) + fragment 5 + lane column 15 (6 * 15)
    assert 96 + 31 + 5 + 90 < t.XROT_ROWS and 4 * t.XROT_ROWS * 16 <= t.TILE_ROWS * 64
