"""Recording (trainer.py --record / --record_dir_name): the reference's camera frames (fly.py:592-610), MI355X-native.

What is recorded: env 0, one chase-camera view, every `time_steps_per_recorded_frame`-th env step.  Poses come out of the
training loop on the device -- the persistent rollout writes them itself (`fly_set_pose_record`), the per-step paths copy
env 0's root / joint angles into the record after each step -- and `fly_render` (csrc/fly_render.hip) turns a batch of
them into RGBA frames.  The host only copies finished frames to pinned memory and hands them to a small fixed pool of
writer threads (PNG, standard library only; zlib releases the GIL).  Recording reads the loop's state and never writes a
buffer the loop reads, so training computes the same bits with it on or off.

Frame files: `<dir>/frame_%06d.png`, the number is the env step s counted since the `Fly` was created (its
`render_count` before the step), for s = 0, k, 2k, ...
"""
import ctypes as C
import os
import queue
import shutil
import struct
import subprocess
import threading
import zlib

import numpy as np
import torch

from . import _lib
from .params import NUM_DOF

WIDTH, HEIGHT = 640, 480
FOV_Y_DEG = 40.0
CAM_OFFSET = (-5.0, -7.0, 4.0)          # mm from (x, y, 0) of the root
LOOK_Z = 1.5                            # the camera looks at (x, y, LOOK_Z)
WRITERS = 4                             # PNG writer threads (fixed: the encode is host-bound, not sized by the machine)
BATCH = 32                              # frames per render launch and device-to-host copy
RING_ROWS = 64                          # pose rows of the per-step record of Fly.step (flushed when full)


def render_config(width=WIDTH, height=HEIGHT, fov_y_deg=FOV_Y_DEG, cam_offset=CAM_OFFSET, look_z=LOOK_Z):
    return _lib.FlyRenderConfig(int(width), int(height), float(fov_y_deg), (C.c_float * 3)(*cam_offset), float(look_z))


def render(fly, poses, rc=None, with_ids=False):
    """fly_render of `poses` (f32 [F, 25] on the env's device) on the current stream: (rgba int32 [F, H, W], ids uint8 or None)."""
    rc = rc if rc is not None else render_config()
    poses = poses.contiguous()
    f = int(poses.shape[0])
    rgba = torch.empty((f, rc.height, rc.width), dtype=torch.int32, device=poses.device)
    ids = torch.empty((f, rc.height, rc.width), dtype=torch.uint8, device=poses.device) if with_ids else None
    _lib.api().fly_render(fly._handle, poses, f, C.byref(rc), rgba, ids, _lib.stream_ptr())
    return rgba, ids


def rgba_to_rgb(rgba):
    """int32 [..., H, W] RGBA dwords (R in the low byte) -> uint8 [..., H, W, 3] (numpy)."""
    a = np.ascontiguousarray(rgba if isinstance(rgba, np.ndarray) else rgba.cpu().numpy())
    return a.view(np.uint8).reshape(a.shape + (4,))[..., :3]


def encode_png(rgb, level=3):
    """uint8 [H, W, 3] -> PNG bytes (colour type 2, 8 bits, filter 0 on every row)."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w, ch = rgb.shape
    if ch != 3:
        raise ValueError("encode_png takes [H, W, 3]")
    raw = np.zeros((h, 1 + 3 * w), np.uint8)
    raw[:, 1:] = rgb.reshape(h, 3 * w)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(raw.tobytes(), level)) + chunk(b"IEND", b""))


def frame_rows(first_step, rows, every):
    """Rows r in [0, rows) of a record whose row r holds env step first_step + r and whose step is a frame step
    (a multiple of `every`)."""
    return list(range((-int(first_step)) % int(every), int(rows), int(every)))


class Recorder:
    """Owns the device pose record, the render launches and the writer pool of one `Fly` (rank 0 only).

    Callers: `capture(row)` copies env 0's current pose into row `row` on the device (per-step paths; captured with the step
    in a hipGraph); `reached(row, step)` tells the host that row `row` now holds env step `step` (rows of one segment are
    consecutive); `flush()` renders the frame rows reached so far and queues them for writing.  A caller flushes before
    anything overwrites rows it has reported (the next rollout's row 0), so only steps the host has run become frames."""

    def __init__(self, fly, dirname, every, rc=None):
        self.fly = fly
        self.dir = dirname
        self.every = max(1, int(every))
        self.rc = rc if rc is not None else render_config()
        os.makedirs(dirname, exist_ok=True)
        self.poses = None
        self._seg = None                         # [first step, first row, rows reached]
        self._q = queue.Queue(maxsize=2 * BATCH)
        self._errors = []
        self._threads = [threading.Thread(target=self._writer, daemon=True) for _ in range(WRITERS)]
        for th in self._threads:
            th.start()
        self.frames_queued = 0
        self._closed = False

    # -- the device record ------------------------------------------------------------------
    def buffer(self, rows):
        """The pose record, [rows, 25] f32 at least (reallocated only when too small; pending frames are flushed first)."""
        if self.poses is None or self.poses.shape[0] < rows:
            self.flush()
            self.poses = torch.zeros((int(rows), _lib.POSE_FLOATS), dtype=torch.float32, device=self.fly.device)
        return self.poses

    def capture(self, row):
        """Device copy of env 0's root position + quaternion and joint angles into pose row `row` (current stream)."""
        p = self.poses[row]
        p[:7].copy_(self.fly.root_tensor[0, :7])
        p[7:].copy_(self.fly.dof_states.view(-1, NUM_DOF, 2)[0, :, 0])

    def next_ring_row(self):
        """Fly.step's record: the row the next step goes to (flushes and starts over when the ring is full)."""
        self.buffer(RING_ROWS)
        row = 0 if self._seg is None else self._seg[1] + self._seg[2]
        if row >= self.poses.shape[0]:
            self.flush()
            row = 0
        return row

    def reached(self, row, step):
        seg = self._seg
        if seg is not None and (row != seg[1] + seg[2] or step != seg[0] + seg[2]):
            self.flush()
            seg = None
        if seg is None:
            self._seg = [int(step), int(row), 1]
        else:
            seg[2] += 1

    # -- frames ------------------------------------------------------------------------------
    def flush(self):
        """Render the frame rows of the current segment, copy them to pinned memory and queue them for the writers."""
        seg, self._seg = self._seg, None
        if seg is None:
            return
        self._raise_errors()
        step0, row0, n = seg
        rows = frame_rows(step0, n, self.every)
        for i in range(0, len(rows), BATCH):
            part = rows[i:i + BATCH]
            sel = self.poses[row0 + part[0]: row0 + part[-1] + 1: self.every]
            rgba, _ = render(self.fly, sel, self.rc)
            host = torch.empty(rgba.shape, dtype=torch.int32, pin_memory=True)
            host.copy_(rgba, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            for j, r in enumerate(part):
                path = os.path.join(self.dir, "frame_%06d.png" % (step0 + r))
                self._q.put((ev, host, j, path))
                self.frames_queued += 1

    def _writer(self):
        while True:
            item = self._q.get()
            try:
                if item is None:
                    return
                ev, host, j, path = item
                ev.synchronize()
                data = encode_png(rgba_to_rgb(host[j].numpy()))
                with open(path, "wb") as f:
                    f.write(data)
            except Exception as e:        # reported on the training thread (flush / close)
                self._errors.append(e)
            finally:
                self._q.task_done()

    def _raise_errors(self):
        if self._errors:
            raise RuntimeError("recording: a frame could not be written: %r" % (self._errors[0],))

    def render_now(self):
        """The frame of env 0's current state, uint8 [H, W, 3] (synchronous; Fly.render())."""
        p = torch.empty((1, _lib.POSE_FLOATS), dtype=torch.float32, device=self.fly.device)
        p[0, :7].copy_(self.fly.root_tensor[0, :7])
        p[0, 7:].copy_(self.fly.dof_states.view(-1, NUM_DOF, 2)[0, :, 0])
        rgba, _ = render(self.fly, p, self.rc)
        return rgba_to_rgb(rgba[0])

    def close(self):
        """Flush what is pending and join the writers (idempotent)."""
        if self._closed:
            return
        self.flush()
        self._closed = True
        for _ in self._threads:
            self._q.put(None)
        for th in self._threads:
            th.join()
        self._raise_errors()

    def generate_video(self):
        """fly.py:592-610: finish the frames; assemble `<dir>.mp4` with ffmpeg when it is on PATH."""
        self.close()
        ffmpeg = shutil.which("ffmpeg")
        out = os.path.normpath(self.dir) + ".mp4"
        if ffmpeg is None:
            print("recorded %d frames to %s (ffmpeg is not on PATH: no video assembled)" % (self.frames_queued, self.dir))
            return None
        fps = max(1.0, 1.0 / (float(self.fly.dt) * self.every))
        subprocess.run([ffmpeg, "-y", "-loglevel", "error", "-framerate", "%g" % fps, "-pattern_type", "glob",
                        "-i", os.path.join(self.dir, "frame_*.png"), "-pix_fmt", "yuv420p", out], check=True)
        print("video: %s (%d frames from %s)" % (out, self.frames_queued, self.dir))
        return out
