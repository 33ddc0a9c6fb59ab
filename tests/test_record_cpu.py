"""CPU: recording's host side -- the standard-library PNG encoder, which env steps become frames, and the renderer's
float64 oracle (tests/render_ref.py) on a pose whose projection is known by hand."""
import math
import struct
import zlib

import numpy as np
import pytest

from fly_bproject_amd.record import encode_png, frame_rows
from tests import render_ref as RR


def decode_png(data):
    """PNG bytes -> uint8 [H, W, 3] (8-bit colour type 2); every chunk's CRC is checked, all five row filters undone."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr, seen_end = 8, b"", None, False
    while pos < len(data):
        (length,) = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + length]
        (crc,) = struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        elif tag == b"IEND":
            seen_end = True
        pos += 12 + length
    assert seen_end and hdr is not None
    w, h, depth, ctype, _, _, interlace = hdr
    assert (depth, ctype, interlace) == (8, 2, 0)
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    out = np.zeros((h, 3 * w), np.int32)
    for y in range(h):
        ft, row = raw[y, 0], raw[y, 1:].astype(np.int32)
        prev = out[y - 1] if y else np.zeros(3 * w, np.int32)
        if ft == 0:
            cur = row
        elif ft == 2:
            cur = (row + prev) & 255
        else:                                  # 1 (sub), 3 (average), 4 (Paeth) depend on the left neighbour
            cur = np.zeros(3 * w, np.int32)
            for x in range(3 * w):
                a = cur[x - 3] if x >= 3 else 0
                b, c = prev[x], (prev[x - 3] if x >= 3 else 0)
                if ft == 1:
                    p = a
                elif ft == 3:
                    p = (a + b) // 2
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[x] = (row[x] + p) & 255
        out[y] = cur
    return out.reshape(h, w, 3).astype(np.uint8)


def test_png_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    img[:5] = 7                                                       # flat rows compress
    data = encode_png(img)
    np.testing.assert_array_equal(decode_png(data), img)
    try:
        from PIL import Image
    except ImportError:
        return
    p = tmp_path / "x.png"
    p.write_bytes(data)
    with Image.open(p) as im:
        assert im.mode == "RGB" and im.size == (53, 37)
        np.testing.assert_array_equal(np.asarray(im), img)


def test_png_rejects_non_rgb():
    with pytest.raises(ValueError):
        encode_png(np.zeros((4, 4, 4), np.uint8))


def test_frame_steps_of_a_rollout_cut_short():
    # a persistent rollout of T = 160 rows starting at env step 320 (every 3rd step a frame); the host stopped after
    # reaching 47 rows (--max_steps): frames only for steps 320 .. 366 that are multiples of 3
    rows = frame_rows(320, 47, 3)
    assert [320 + r for r in rows] == [s for s in range(320, 367) if s % 3 == 0]
    assert frame_rows(0, 0, 2) == []
    # a whole run of 167 steps in rollouts of 160: exactly frames 0, 3, ..., 165
    steps = [160 * k + r for k, n in ((0, 160), (1, 7)) for r in frame_rows(160 * k, n, 3)]
    assert steps == list(range(0, 166, 3))


def _rest_pose(params, z):
    pose = np.zeros(25)
    pose[2], pose[6] = z, 1.0
    pose[7:] = params.dof_pose[:]
    return pose


def test_oracle_root_projects_to_the_image_centre():
    from fly_bproject_amd.params import default_params
    p = default_params(32)
    look_z = 1.5
    pose = _rest_pose(p, look_z)                    # the root sits at the camera's look-at point
    pose[0], pose[1] = 12.5, -3.0
    w, h = 96, 72
    u, v = RR.project(pose[:3], pose, w, h, 40.0, (-5.0, -7.0, 4.0), look_z)
    assert abs(u - w / 2) < 1e-9 and abs(v - h / 2) < 1e-9
    rgb, ids = RR.render(p, pose, w, h, 40.0, (-5.0, -7.0, 4.0), look_z)
    assert (ids[h // 2 - 1:h // 2 + 1, w // 2 - 1:w // 2 + 1] == RR.RID_BODY).all()     # the thorax, around the centre
    assert ids[0, 0] == RR.RID_SKY and ids[-1, 0] == RR.RID_GROUND
    # a point one mm along the camera's right axis projects right of the centre by f = (w / 2) / (tan(fov/2) * aspect) / dist
    cam, fw, rt, up = RR.camera(pose, w, h, 40.0, (-5.0, -7.0, 4.0), look_z)
    dist = np.linalg.norm(pose[:3] - cam)
    u2, v2 = RR.project(pose[:3] + rt, pose, w, h, 40.0, (-5.0, -7.0, 4.0), look_z)
    assert abs(u2 - (w / 2 + (w / 2) / (math.tan(math.radians(20.0)) * w / h) / dist)) < 1e-9 and abs(v2 - h / 2) < 1e-9
    # sky pixels carry the sky colour unshaded
    assert tuple(rgb[0, 0]) == tuple(int(math.floor(c * 255 + 0.5)) for c in RR.SKY_RGB)
