"""The streaming pipeline of test_video: YUV4MPEG2 frames from a source through a net to a sink, for
nets that look at one frame (temporal radius R = 0, the picture models) and at 2 R + 1 frames (R = 1, VESPCN).

Output frame t comes from frames max(t - R, 0) .. min(t + R, T - 1) of the stream, and the net sees whole batches.  An
input slot holds video_batch + 2 R frames: [2 R carries, k fresh frames].  The carries are the last 2 R frames of the
previous slot; in the first slot they are replicas of the stream's first frame.  A read that comes back short
(k < video_batch, 0 included) has seen the end of the stream and puts R replicas of the last frame behind the fresh ones.
So the output lags the input by R frames, and with R > 0 a final empty read flushes the last ones.  video_window and
video_window_fill are pure host code (tests/test_vespcn_cpu.py drives them with frame numbers in place of frames)."""
import queue
import threading
import time

import torch

from . import data, ops

SLOTS = 3   # pinned + device buffers per direction: one being filled, one in flight, one being consumed


def video_window(k, first, last, radius):
    """One read of the schedule: k fresh frames, `first` read of the stream, `last` (the read came back short).
    -> (m, lo, n): the slot's first m frames are in use, the windows are slot[j - radius : j + radius + 1] for the n
    centres j = lo .. lo + n - 1.  n may be 0: a first read of no more than `radius` frames that is not the last, or with
    radius 0 the empty read behind a stream whose length is a multiple of the batch."""
    m = 2 * radius + k + (radius if last else 0)
    lo = 2 * radius if first else radius
    return m, lo, max(m - radius - lo, 0)


def video_window_fill(slot, prev, k, kprev, first, last, radius):
    """Completes a slot whose fresh frames lie at slot[2 * radius : 2 * radius + k]: the carries (from `prev`, the previous
    slot with its kprev fresh frames; replicas of the first frame in the first read) and the end's replicas.  slot, prev:
    anything indexable by frame whose rows can be assigned (pinned uint8 tensors, numpy arrays)."""
    if first and k == 0:
        raise ValueError("test_video: the stream holds no frame")
    for j in range(2 * radius):
        slot[j] = slot[2 * radius] if first else prev[kprev + j]
    if last:
        for j in range(radius):
            slot[2 * radius + k + j] = slot[2 * radius + k - 1]


def _video_pack(y, frames, lay, out_lay, out):
    """The net's output y -> the packed output frames `out`, one yuv_pack launch; a Y model's Cb / Cr come from the
    input frames through the 8-bit bicubic resizer, to the chroma size of what the net actually returned."""
    chroma = None
    if int(y.shape[1]) == 1 and lay.sub != "mono":
        chroma = ops.yuv_chroma(frames, lay, out_lay.ch, out_lay.cw)
    ops.yuv_pack(y, out_lay, chroma, out=out)


def _take(q):
    item = q.get()
    if isinstance(item, BaseException):   # from the reader's or the writer's thread
        raise item
    return item


def run(src, dst, n_max, radius, net, num_channels, device, trace=None):
    """The stream `src` through `net` to `dst` in reads of n_max frames -> (frames written, input layout, output layout,
    seconds).  net(x, lo, n): the unpacked slot x [m,C,H,W] (fp32, on the device) -> the fp32 output [n,C,OH,OW] for the
    frames lo .. lo + n - 1 of x; it may look at `radius` frames of x on either side of them.
    A reader thread fills SLOTS pinned buffers and completes their windows; uploads, compute and downloads run on three
    streams joined by events; a writer thread drains SLOTS pinned buffers.  Nothing waits for the whole device, and
    every buffer is made once (the output side when the first output has shown the net's output size).  A read that
    yields no output (video_window) starts nothing on the device.  trace: a list that gets torch.cuda.memory_allocated()
    at the end of every read that brought a frame or produced one."""
    reader = data.Y4MReader(src)
    lay = reader.layout
    pin_in = [torch.empty((n_max + 2 * radius, lay.frame_bytes), dtype=torch.uint8, pin_memory=True) for _ in range(SLOTS)]
    dev_in = [torch.empty((n_max + 2 * radius, lay.frame_bytes), dtype=torch.uint8, device=device) for _ in range(SLOTS)]
    pin_out = dev_out = out_lay = writer = write_thread = None
    h2d, comp, d2h = (torch.cuda.Stream(device) for _ in range(3))
    ev_up, ev_in_used, ev_packed, ev_down = ([torch.cuda.Event() for _ in range(SLOTS)] for _ in range(4))
    free_in, filled, free_out, to_write = (queue.Queue() for _ in range(4))
    for i in range(SLOTS):
        free_in.put(i)
        free_out.put(i)

    def read_loop():
        # the only writer of the pinned input buffers, and it fills them in order: the previous slot is its own to keep
        prev, kprev, first = None, 0, True
        try:
            while True:
                i = free_in.get()
                if i is None:
                    return
                ev_up[i].synchronize()   # its last upload has left the pinned buffer
                k = reader.read_into(pin_in[i][2 * radius:2 * radius + n_max], n_max)
                last = k < n_max
                video_window_fill(pin_in[i], prev, k, kprev, first, last, radius)
                filled.put((i, k, first, last))
                if last:
                    return
                prev, kprev, first = pin_in[i], k, False
        except BaseException as e:   # handed to the caller's thread
            filled.put(e)

    def write_loop():
        try:
            while True:
                item = to_write.get()
                if item is None:
                    return
                o, n = item
                ev_down[o].synchronize()
                writer.write(pin_out[o], n)
                free_out.put(o)
        except BaseException as e:
            free_out.put(e)

    frames_done = 0
    t0 = time.perf_counter()
    cur = torch.cuda.current_stream()
    for s in (h2d, comp, d2h):
        s.wait_stream(cur)
    read_thread = threading.Thread(target=read_loop, name="y4m-reader", daemon=True)
    read_thread.start()
    try:
        while True:
            i, k, first, last = _take(filled)
            m, lo, n = video_window(k, first, last, radius)
            if n:
                with torch.cuda.stream(h2d):
                    h2d.wait_event(ev_in_used[i])
                    dev_in[i][:m].copy_(pin_in[i][:m], non_blocking=True)
                    ev_up[i].record(h2d)
                with torch.cuda.stream(comp):
                    comp.wait_event(ev_up[i])
                    x = ops.yuv_unpack(dev_in[i][:m], lay, num_channels)
                    y = net(x, lo, n)
                    if y.dim() != 4 or int(y.shape[0]) != n or int(y.shape[1]) != num_channels:
                        raise RuntimeError("test_video: the net returned %s for a batch of %d frames of %d channel(s)"
                                           % (tuple(y.shape), n, num_channels))
                    if out_lay is None:   # the first output shows the net's output size: the output side is made now
                        out_lay = ops.yuv_layout(int(y.shape[-1]), int(y.shape[-2]), lay.sub,
                                                 "the net's output for a %s stream" % (reader.header.chroma_tag or "C420jpeg"))
                        writer = data.Y4MWriter(dst, reader.header.scaled(out_lay.W, out_lay.H))
                        pin_out = [torch.empty((n_max, out_lay.frame_bytes), dtype=torch.uint8, pin_memory=True) for _ in range(SLOTS)]
                        dev_out = [torch.empty((n_max, out_lay.frame_bytes), dtype=torch.uint8, device=device) for _ in range(SLOTS)]
                        write_thread = threading.Thread(target=write_loop, name="y4m-writer", daemon=True)
                        write_thread.start()
                    o = _take(free_out)   # the writer has drained it, so its last download is over
                    _video_pack(y, dev_in[i][lo:lo + n], lay, out_lay, dev_out[o][:n])
                    ev_in_used[i].record(comp)
                    ev_packed[o].record(comp)
                    del x, y
            if trace is not None and (k or n):
                trace.append(torch.cuda.memory_allocated(device))
            free_in.put(i)
            if n:
                with torch.cuda.stream(d2h):
                    d2h.wait_event(ev_packed[o])
                    pin_out[o][:n].copy_(dev_out[o][:n], non_blocking=True)
                    ev_down[o].record(d2h)
                to_write.put((o, n))
                frames_done += n
            if last:
                break
        to_write.put(None)
        write_thread.join()
        for item in list(free_out.queue):   # the drained slots, or the writer's exception
            if isinstance(item, BaseException):
                raise item
        read_thread.join()   # it has seen the end of the stream
    finally:   # the end of the call, not its steady state (on an error the reader may sit in a read: it is a daemon)
        free_in.put(None)
        to_write.put(None)
        if write_thread is not None:
            write_thread.join()
        for s in (h2d, comp, d2h):
            s.synchronize()
        reader.close()
        if writer is not None:
            writer.close()
    return frames_done, lay, out_lay, time.perf_counter() - t0
