"""CPU tests of what the item-list entries share: csrc/item_list.h through its host check program, and item_lists.py.

The host program (tests/host/item_list_check.cpp) is the test of the arena-fit predicate: it is built host-only, with the compiler that
builds the library, under -fsanitize=undefined,address -fno-sanitize-recover=all -- a signed overflow in a check ends the program --
and asserts the predicate and the host helpers at their boundaries, offsets next to 2^63 among them.
"""
import os
import subprocess

import pytest
import torch

from grl_image_restoration_amd import item_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_the_fit_predicate_and_the_host_helpers_under_sanitizers(tmp_path):
    exe = str(tmp_path / "item_list_check")
    san = ["-Xarch_host", "-fsanitize=undefined,address", "-Xarch_host", "-fno-sanitize-recover=all"]
    src = os.path.join(ROOT, "tests", "host", "item_list_check.cpp")
    build = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *san, src, "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr


def test_pack_views_and_table():
    g = torch.Generator().manual_seed(0)
    xs = [torch.rand(3, 2, 5, generator=g), torch.rand(3, 1, 1, generator=g), torch.rand(3, 4, 3, generator=g)]
    arena, offs = item_lists.pack(xs)
    assert offs == [0, 30, 33] and arena.shape == (69,)
    assert all(torch.equal(v, x) for v, x in zip(item_lists.views(arena, offs, [x.shape for x in xs]), xs))
    arena, offs = item_lists.pack(xs, align=4)
    assert offs == [0, 32, 36] and arena.shape == (72,) and not arena[30:32].any() and not arena[35:36].any()
    assert all(torch.equal(v, x) for v, x in zip(item_lists.views(arena, offs, [x.shape for x in xs]), xs))
    out, offs = item_lists.empty([(3, 2, 2), (4, 4), (1, 7, 1)], "cpu")
    assert offs == [0, 12, 28] and out.shape == (35,) and out.dtype == torch.float32
    t = item_lists.table([(0, 1, 2, 3, 4, 5, 6, 7), (8, 9, 10, 11, 12, 13, 14, 2 ** 40)], "cpu")
    assert t.shape == (2, 8) and t.dtype == torch.int64 and t[1, 7] == 2 ** 40


def test_check_images():
    x = torch.rand(3, 4, 5)
    item_lists.check_images([x, torch.rand(3, 1, 9)], "f")
    item_lists.check_images([x[:1]], "f")
    item_lists.check_images([x.double()], "f", (3,), 3)
    for bad, kw in (([], {}), ([x, x[:1]], {}), ([x[:2]], {}), ([x[0]], {}), ([x.numpy()], {}), ([x, x.double()], {}),
                    ([x[:1]], dict(channels=(3,))), ([x[:, :2]], dict(min_side=3)), ([torch.rand(3, 0, 4)], {})):
        with pytest.raises(ValueError, match="^f: "):
            item_lists.check_images(bad, "f", **kw)
    with pytest.raises(ValueError, match=r"\(3, h, w\)"):
        item_lists.check_images([x[:1]], "f", (3,))
    with pytest.raises(ValueError, match="at least 3"):
        item_lists.check_images([x[:, :2]], "f", (3,), 3)
