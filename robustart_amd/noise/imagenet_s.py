"""ImageNet-S ("system noise": decoder x resize operator) -- drop-in for add_noise_for_imagenet_s /
ImageTransfer(return_online=True) (RobustART/noise/utils/add_noise_utils.py:34-38, imagenet_s_gen.py:38-279).

Decoding a file is host I/O (PIL, as the reference's 'pil' decoder); the resize operator -- the part that differs
between the ImageNet-S variants and the part that is arithmetic -- runs on the GPU, bit-exact with Pillow, through
rart_pil_resize_u8; the five 'opencv-*' operators run through rart_cv_resize_u8, a restatement of OpenCV's resize.cpp
(OpenCV is not installed here, so those five are parity-unpinned -- see oracle/resize_cv_np.py).  Not available in this
build (raise NotImplementedError, loudly): the 'opencv' and 'ffmpeg' decoders and the reference's memcached reader.  Unlike the reference (which passes float sizes to Image.resize and only works on
Python <= 3.9, imagenet_s_gen.py:129,167) sizes are converted with int().
pil_resize_batch is the batched form of pil_resize for images of different sizes -- crop(box), resize, crop window, mirror for a whole
batch in one rart_resize_batch_u8 call -- cv_resize_batch the same for cv_resize through rart_cv_resize_batch_u8 (each
image takes the code cv2.resize chooses for its size), and image_transfer_batch the batch form of image_transfer on top of the two.
decode_batch_gpu is the batched form of the 'pil' decoder for baseline JPEG files: Huffman decoding on host threads, the arithmetic in
rart_jpeg_decode_u8, the same bytes as Pillow; FileImageNet(reader='hip') reads through it.  entropy='gpu' moves the
Huffman decoding to the GPU too (rart_jpeg_entropy_decode_gpu), bit-identical to the host decoder; 'host' is the default."""
import random

import numpy as np

from .. import _lib

PIL_FILTERS = {'pil-nearest': 0, 'pil-bilinear': 1, 'pil-cubic': 2, 'pil-box': 3, 'pil-hamming': 4, 'pil-lanczos': 5}
# imagenet_s_gen.py:27-33 -> cv2.INTER_* constants
CV_MODES = {'opencv-nearest': 0, 'opencv-bilinear': 1, 'opencv-cubic': 2, 'opencv-area': 3, 'opencv-lanczos': 4}


def pil_resize(batch_u8, resize_hw, filter_id, crop=None):
    """batch_u8: CUDA uint8 (n,h,w,3) -> CUDA uint8 (n, ch, cw, 3) = Image.resize((rw, rh), filter) then crop
    (cy, cx, ch, cw); crop=None keeps the whole resized image."""
    torch = _lib.require_gpu()
    lib = _lib.load()
    n, h, w, _ = batch_u8.shape
    rh, rw = int(resize_hw[0]), int(resize_hw[1])
    cy, cx, ch, cw = crop if crop is not None else (0, 0, rh, rw)
    out = torch.empty(n, ch, cw, 3, dtype=torch.uint8, device=batch_u8.device)
    nb = lib.rart_pil_resize_workspace_bytes(n, h, w, rh, rw, filter_id, cy, cx, ch, cw)
    ws = _lib.workspace(nb, batch_u8.device)
    _lib.check(lib.rart_pil_resize_u8(_lib.ptr(batch_u8), _lib.ptr(out), n, h, w, rh, rw, filter_id, cy, cx, ch, cw,
                                      _lib.ptr(ws), nb, _lib.stream_ptr()))
    return out


def cv_resize(batch_u8, resize_hw, interpolation, crop=None):
    """batch_u8: CUDA uint8 (n,h,w,3) -> cv2.resize(img, (rw, rh), interpolation) then crop (cy, cx, ch, cw)."""
    torch = _lib.require_gpu()
    lib = _lib.load()
    n, h, w, _ = batch_u8.shape
    rh, rw = int(resize_hw[0]), int(resize_hw[1])
    cy, cx, ch, cw = crop if crop is not None else (0, 0, rh, rw)
    out = torch.empty(n, ch, cw, 3, dtype=torch.uint8, device=batch_u8.device)
    nb = lib.rart_cv_resize_workspace_bytes(n, h, w, rh, rw, interpolation, cy, cx, ch, cw)
    ws = _lib.workspace(nb, batch_u8.device)
    _lib.check(lib.rart_cv_resize_u8(_lib.ptr(batch_u8), _lib.ptr(out), n, h, w, rh, rw, interpolation, cy, cx, ch, cw,
                                     _lib.ptr(ws), nb, _lib.stream_ptr()))
    return out


_plan_pinned = {}          # device -> (pinned plan buffer, the event of the last copy that read it)
resize_batch_launches = 0  # rart_resize_batch_u8 calls made by pil_resize_batch (one per call, whatever the batch holds)


def pil_resize_batch(images, resize_hw, filter_id, crop=None, boxes=None, flips=None, out=None):
    """images: a list of n CUDA uint8 HxWx3 tensors of any sizes (views of decode_batch_gpu's packed buffer or separate
    allocations) -> CUDA uint8 (n, ch, cw, 3): per image Image.crop(box).resize((rw, rh), filter), the crop window (cy, cx, ch, cw)
    of it, then a left-right mirror where flips[k].  boxes[k] = (y, x, h, w) inside image k (None: the whole image; the box is a
    hard boundary, unlike Image.resize(box=...)); crop=None keeps the whole resized image; out: the tensor to fill.
    One rart_resize_batch_plan call on the host, one copy of its buffer (pinned, kept between calls), one rart_resize_batch_u8
    call: two launches, one for NEAREST."""
    return _resize_batch('pil_resize_batch', images, resize_hw, filter_id, crop, boxes, flips, out)


cv_resize_batch_launches = 0   # rart_cv_resize_batch_u8 calls made by cv_resize_batch (one per call, whatever the batch holds)


def cv_resize_batch(images, resize_hw, interpolation, crop=None, boxes=None, flips=None, out=None):
    """The batched form of cv_resize for images of different sizes, the counterpart of pil_resize_batch (same arguments):
    -> CUDA uint8 (n, ch, cw, 3), image k equal to cv_resize(images[k][box][None], resize_hw, interpolation, crop)[0], mirrored
    left-right where flips[k].  boxes[k] = (y, x, h, w) inside image k (None: the whole image) is a hard boundary: edge taps
    replicate the box's border.  cv2.resize chooses its code from the source size, so the images of one call may each take
    another path (nearest, two-pass, float area, integer area).
    One rart_cv_resize_batch_plan call on the host, one copy of its buffer (pinned, kept between calls), one
    rart_cv_resize_batch_u8 call: two launches, one when no image takes the two-pass path."""
    return _resize_batch('cv_resize_batch', images, resize_hw, interpolation, crop, boxes, flips, out)


# who -> (descriptor, plan header, plan entry, device entry, the module counter of device-entry calls)
_BATCH_ENTRIES = {
    'pil_resize_batch': ('ResizeDesc', 'ResizePlan', 'rart_resize_batch_plan', 'rart_resize_batch_u8', 'resize_batch_launches'),
    'cv_resize_batch': ('CvResizeDesc', 'CvResizePlan', 'rart_cv_resize_batch_plan', 'rart_cv_resize_batch_u8', 'cv_resize_batch_launches'),
}


def _resize_batch(who, images, resize_hw, mode, crop, boxes, flips, out):
    """pil_resize_batch / cv_resize_batch: the two entry pairs take the same arguments and the same plan buffer."""
    import ctypes
    torch = _lib.require_gpu()
    lib = _lib.load()
    desc_t, plan_t, plan_fn, run_fn, counter = _BATCH_ENTRIES[who]
    plan_fn, run_fn = getattr(lib, plan_fn), getattr(lib, run_fn)
    images = list(images)
    n = len(images)
    rh, rw = int(resize_hw[0]), int(resize_hw[1])
    cy, cx, ch, cw = (int(v) for v in (crop if crop is not None else (0, 0, rh, rw)))
    if n == 0:
        raise ValueError('%s: an empty list of images' % who)
    dev = images[0].device
    descs = (getattr(_lib, desc_t) * n)()
    for k, img in enumerate(images):
        if not (isinstance(img, torch.Tensor) and img.is_cuda and img.device == dev and img.dtype == torch.uint8 and img.dim() == 3
                and img.shape[2] == 3 and img.is_contiguous()):
            raise ValueError('%s: image %d must be a contiguous CUDA uint8 HxWx3 tensor on %s' % (who, k, dev))
        d = descs[k]
        d.src, d.h, d.w = img.data_ptr(), img.shape[0], img.shape[1]
        d.box_y, d.box_x, d.box_h, d.box_w = (int(v) for v in boxes[k]) if boxes is not None and boxes[k] is not None else (0, 0, d.h, d.w)
        d.flip = int(bool(flips[k])) if flips is not None else 0
    if out is None:
        out = torch.empty(n, ch, cw, 3, dtype=torch.uint8, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dev and out.dtype == torch.uint8
              and tuple(out.shape) == (n, ch, cw, 3) and out.is_contiguous()):
        raise ValueError('%s: out must be a contiguous CUDA uint8 tensor of shape %r on %s' % (who, (n, ch, cw, 3), dev))
    with torch.cuda.device(dev):
        host, ev = _plan_pinned.pop(dev, (None, None))     # taken out while in use, as decode_batch_gpu does
        if ev is not None:
            ev.synchronize()               # the previous call's copy has left the buffer
        if host is None:
            host = torch.empty(1 << 20, dtype=torch.uint8, pin_memory=True)
        sizes = getattr(_lib, plan_t)()
        args = (ctypes.addressof(descs), n, mode, rh, rw, cy, cx, ch, cw)
        st = plan_fn(*args, host.data_ptr(), host.numel(), ctypes.byref(sizes))
        if st == 3:                        # RART_ERR_WORKSPACE: `sizes` says what the plan needs
            host = torch.empty(int(sizes.total_bytes * 1.25), dtype=torch.uint8, pin_memory=True)
            st = plan_fn(*args, host.data_ptr(), host.numel(), ctypes.byref(sizes))
        _lib.check(st)
        total = int(sizes.total_bytes)
        plan = torch.empty(total, dtype=torch.uint8, device=dev)
        plan.copy_(host[:total], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        ws = _lib.workspace(int(sizes.workspace_bytes), dev)
        globals()[counter] += 1
        try:
            _lib.check(run_fn(_lib.ptr(plan), host.data_ptr(), total, _lib.ptr(ws), int(sizes.workspace_bytes), _lib.ptr(out),
                              out.numel(), _lib.stream_ptr()))
        finally:
            _plan_pinned[dev] = (host, ev)
    return out


def decode(path_or_bytes, decoder_type='pil'):
    """imagenet_s_gen.py:177-196 ('pil' branch): RGB uint8 array."""
    if decoder_type != 'pil':
        raise NotImplementedError("decoder_type %r needs OpenCV / ffmpeg, which this build does not have; only 'pil' is "
                                  "available" % (decoder_type,))
    import io
    from PIL import Image
    src = io.BytesIO(path_or_bytes) if isinstance(path_or_bytes, (bytes, bytearray)) else path_or_bytes
    with Image.open(src) as img:
        return np.array(img.convert('RGB'))


def jpeg_probe(data):
    """rart_jpeg_probe on encoded bytes (host only) -> _lib.JpegInfo; info.status is 0 when the file is in the supported set
    (baseline, one scan, grayscale or YCbCr 4:4:4 / 4:2:2 / 4:2:0), 2 when Pillow has to decode it."""
    import ctypes
    info = _lib.JpegInfo()
    _lib.load().rart_jpeg_probe(data, len(data), ctypes.byref(info))
    return info


def jpeg_entropy_decode(data, info, coef):
    """rart_jpeg_entropy_decode (host only): the scan's coefficients into `coef`, a C-contiguous int16 numpy array of at least
    info.coef_count elements -- per component, block-row-major, 64 per block in natural order, not dequantised.  -> status"""
    import ctypes
    assert coef.dtype == np.int16 and coef.flags['C_CONTIGUOUS']
    return _lib.load().rart_jpeg_entropy_decode(data, len(data), ctypes.byref(info), coef.ctypes.data, coef.size)


def _read_bytes(item):
    if isinstance(item, (bytes, bytearray, memoryview)):
        return bytes(item)
    with open(item, 'rb') as f:
        return f.read()


_pinned = {}               # device -> (pinned staging buffer, the event of the last copy that read it)
MAX_DECODE_WORKERS = 16
decode_launches = 0        # rart_jpeg_decode_u8 calls made by decode_batch_gpu (one per batch that has a GPU-decodable file)


entropy_launches = 0       # rart_jpeg_entropy_decode_gpu calls made by decode_batch_gpu(entropy='gpu'): one per batch that has a
#                            file for the device entropy decoder
entropy_stats = {'gpu': 0, 'host_dri': 0, 'host_not_converged': 0, 'invalid': 0}   # images by who decoded their entropy data
ENTROPY_MODES = ('host', 'gpu')
entropy_params = {'subseq_bytes': 0, 'max_rounds': 0}   # what decode_batch_gpu(entropy='gpu') uses where its caller passes 0
#                                                         (FileImageNet does); 0 = the library's defaults


def check_entropy_mode(entropy):
    if entropy not in ENTROPY_MODES:
        raise ValueError("entropy must be 'host' or 'gpu', got %r" % (entropy,))
    return entropy


def jpeg_scan_plan(data, info, subseq_bytes=0):
    """rart_jpeg_scan_plan (host only) -> (_lib.JpegScan, the image's Huffman tables as a ctypes byte array of
    JPEG_MAX_TABLES * JPEG_HUFF_PITCH bytes, of which scan.ntab * JPEG_HUFF_PITCH are written)"""
    import ctypes
    scan = _lib.JpegScan()
    tabs = (ctypes.c_ubyte * (_lib.JPEG_MAX_TABLES * _lib.JPEG_HUFF_PITCH))()
    _lib.check(_lib.load().rart_jpeg_scan_plan(data, len(data), ctypes.byref(info), subseq_bytes, ctypes.byref(scan), tabs, len(tabs)))
    return scan, tabs


def jpeg_entropy_emulate(data, info, coef, subseq_bytes=0, max_rounds=0):
    """rart_jpeg_entropy_emulate (host only): the device entropy decoder's rounds, prefix sums and write pass on the CPU.
    coef as for jpeg_entropy_decode.  -> (status, rounds_used)"""
    import ctypes
    assert coef.dtype == np.int16 and coef.flags['C_CONTIGUOUS']
    used = ctypes.c_int32(0)
    st = _lib.load().rart_jpeg_entropy_emulate(data, len(data), ctypes.byref(info), subseq_bytes, max_rounds, coef.ctypes.data, coef.size,
                                               ctypes.byref(used))
    return st, used.value


def _fill_jpeg_descs(descs, infos):
    """the rart_jpeg_desc of each probed image, in the order given -> (blocks, pixels)"""
    blk = pix = plane = 0
    for j, info in enumerate(infos):
        d = descs[j]
        d.height, d.width, d.ncomp = info.height, info.width, info.ncomp
        d.h_samp, d.v_samp = info.h_samp[0], info.v_samp[0]
        d.qt_off, d.out_off = j * 192, 3 * pix
        for c in range(3):
            bw, bh = (info.blocks_w[c], info.blocks_h[c]) if c < info.ncomp else (0, 0)
            d.blocks_w[c], d.blocks_h[c], d.block_start[c] = bw, bh, blk
            d.plane_off[c] = plane
            blk += bw * bh
            plane += (bw * bh * 64 + 15) // 16 * 16
        pix += info.height * info.width
    return blk, pix


def _align16(v):
    return (v + 15) // 16 * 16


def _pool_map(pool, fn, seq, workers):
    """pool.map(fn, seq) in slices of about a quarter of a worker's share: the per-file steps of the GPU entropy path are tens of
    microseconds each, less than what one future costs"""
    seq = list(seq)
    step = max(1, -(-len(seq) // (4 * workers)))
    parts = pool.map(lambda part: [fn(x) for x in part], [seq[i:i + step] for i in range(0, len(seq), step)])
    return [r for part in parts for r in part]


def _decode_batch_gpu_entropy(items, workers, timings, subseq_bytes, max_rounds):
    """decode_batch_gpu(entropy='gpu'): the pool reads, probes and plans; one pinned buffer holds descriptors | scan descriptors |
    quantisation tables | Huffman tables | scan bytes | the coefficients of host-path images (restart intervals, scans beyond the
    kernel's limits), which come first in the batch's block numbering; one copy moves it; rart_jpeg_entropy_decode_gpu fills the
    other images' coefficients behind them; the status array comes back (the batch's one synchronisation); images that have
    not converged are decoded by rart_jpeg_entropy_decode into their slots; rart_jpeg_decode_u8 finishes the whole batch."""
    global decode_launches, entropy_launches
    import ctypes
    import time
    from concurrent.futures import ThreadPoolExecutor
    torch = _lib.require_gpu()
    lib = _lib.load()
    n = len(items)
    t0 = time.perf_counter()

    def probe(item):
        data = _read_bytes(item)
        info = jpeg_probe(data)
        return (data, info) + (jpeg_scan_plan(data, info, subseq_bytes) if info.status == 0 else (None, None))

    images, used = [None] * n, [False] * n
    with ThreadPoolExecutor(max_workers=workers) as pool:
        probed = _pool_map(pool, probe, items, workers)
        ok_ids = [k for k in range(n) if probed[k][1].status == 0]
        ids = [k for k in ok_ids if probed[k][2].host_path] + [k for k in ok_ids if not probed[k][2].host_path]
        if ids:
            m = len(ids)
            m_host = sum(1 for k in ids if probed[k][2].host_path)
            descs = (_lib.JpegDesc * m)()
            scans = (_lib.JpegScan * m)()
            blk, pix = _fill_jpeg_descs(descs, [probed[k][1] for k in ids])
            host_blk = descs[m_host].block_start[0] if m_host < m else blk
            tab_bytes = scan_bytes = sub = 0
            for j, k in enumerate(ids):
                s = scans[j]
                ctypes.memmove(ctypes.addressof(s), ctypes.addressof(probed[k][2]), ctypes.sizeof(s))
                s.block_start, s.sub_start, s.tab_off, s.scan_off = descs[j].block_start[0], sub, tab_bytes, scan_bytes
                sub += s.nsub
                tab_bytes += s.ntab * _lib.JPEG_HUFF_PITCH
                scan_bytes += _align16(s.scan_len)
            # staging: descriptors | scan descriptors | quantisation tables | Huffman tables | scan bytes | host-path coefficients;
            # on the device the other images' coefficients, then status and rounds_used, follow.  Each region 16-byte aligned.
            o_scan = _align16(ctypes.sizeof(descs))
            o_qt = o_scan + _align16(ctypes.sizeof(scans))
            o_tab = o_qt + m * 192 * 2
            o_bytes = o_tab + max(tab_bytes, 16)
            o_coef = o_bytes + max(scan_bytes, 16)
            staged = o_coef + host_blk * 128
            o_status = o_coef + blk * 128
            total = o_status + _align16(8 * m)
            dev = torch.device('cuda', torch.cuda.current_device())
            host, ev = _pinned.pop(dev, (None, None))
            if ev is not None:
                ev.synchronize()
            if host is None or host.numel() < staged:
                host = torch.empty(int(staged * 1.25), dtype=torch.uint8, pin_memory=True)
            hnp = host.numpy()
            ctypes.memmove(hnp.ctypes.data, ctypes.addressof(descs), ctypes.sizeof(descs))
            ctypes.memmove(hnp.ctypes.data + o_scan, ctypes.addressof(scans), ctypes.sizeof(scans))
            qt = hnp[o_qt:o_tab].view(np.uint16).reshape(m, 3, 64)
            coef = hnp[o_coef:staged].view(np.int16)

            def stage(j):
                data, info, _, tabs = probed[ids[j]]
                s = scans[j]
                qt[j] = np.ctypeslib.as_array(info.qt)
                if s.host_path:
                    lo = descs[j].block_start[0] * 64
                    return jpeg_entropy_decode(data, info, coef[lo:lo + info.coef_count])
                nt = s.ntab * _lib.JPEG_HUFF_PITCH
                ctypes.memmove(hnp.ctypes.data + o_tab + s.tab_off, tabs, nt)
                hnp[o_bytes + s.scan_off:o_bytes + s.scan_off + s.scan_len] = np.frombuffer(data, np.uint8, s.scan_len, s.scan_pos)
                return 0

            status = _pool_map(pool, stage, range(m), workers)
            if timings is not None:
                timings['host_s'] = time.perf_counter() - t0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            dbuf = torch.empty(total, dtype=torch.uint8, device=dev)
            dbuf[:staged].copy_(host[:staged], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            _pinned[dev] = (host, ev)
            if timings is not None:
                torch.cuda.synchronize()
                timings['copy_s'] = time.perf_counter() - t0
                t0 = time.perf_counter()
            base = dbuf.data_ptr()
            if m_host < m:
                nb = lib.rart_jpeg_entropy_workspace_bytes(ctypes.addressof(scans), m)
                ws = _lib.workspace(nb, dev)
                entropy_launches += 1
                if timings is not None:
                    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ev0.record()
                _lib.check(lib.rart_jpeg_entropy_decode_gpu(base + o_scan, ctypes.addressof(scans), m, base + o_bytes, max(scan_bytes, 16),
                                                            base + o_tab, max(tab_bytes, 16), base + o_coef, blk, subseq_bytes, max_rounds,
                                                            base + o_status, base + o_status + 4 * m, _lib.ptr(ws), nb, _lib.stream_ptr()))
                if timings is not None:
                    ev1.record()
                dev_status = dbuf[o_status:o_status + 4 * m].view(torch.int32).cpu().tolist()   # the batch's one synchronisation
                if timings is not None:
                    timings['entropy_kernel_s'] = 1e-3 * ev0.elapsed_time(ev1)         # the memset + the launch, by device events
                redo = [j for j in range(m_host, m) if dev_status[j] == 2]

                def fallback(j):
                    data, info = probed[ids[j]][:2]
                    tmp = np.empty(info.coef_count, np.int16)
                    return jpeg_entropy_decode(data, info, tmp), tmp

                for j, (st, tmp) in zip(redo, pool.map(fallback, redo)):
                    lo = o_coef + descs[j].block_start[0] * 128
                    dbuf[lo:lo + tmp.nbytes].copy_(torch.from_numpy(tmp).view(torch.uint8))
                    dev_status[j] = st
                for j in range(m_host, m):
                    status[j] = dev_status[j]
                entropy_stats['host_not_converged'] += len(redo)
                entropy_stats['gpu'] += sum(1 for j in range(m_host, m) if status[j] == 0) - sum(1 for j in redo if status[j] == 0)
            entropy_stats['host_dri'] += m_host
            entropy_stats['invalid'] += sum(1 for j in range(m) if status[j] != 0)
            if timings is not None:
                torch.cuda.synchronize()
                timings['entropy_s'] = time.perf_counter() - t0
                t0 = time.perf_counter()
            out = torch.empty(3 * pix, dtype=torch.uint8, device=dev)
            nb = lib.rart_jpeg_decode_workspace_bytes(ctypes.addressof(descs), m)
            ws = _lib.workspace(nb, dev)
            decode_launches += 1
            _lib.check(lib.rart_jpeg_decode_u8(base, ctypes.addressof(descs), m, base + o_coef, blk, base + o_qt, m * 192, _lib.ptr(ws), nb,
                                               _lib.ptr(out), out.numel(), _lib.stream_ptr()))
            if timings is not None:
                torch.cuda.synchronize()
                timings['device_s'] = time.perf_counter() - t0
            for j, k in enumerate(ids):
                if status[j] == 0:
                    d = descs[j]
                    images[k] = out[d.out_off:d.out_off + 3 * d.height * d.width].view(d.height, d.width, 3)
                    used[k] = True
    for k in range(n):
        if images[k] is None:
            images[k] = torch.from_numpy(decode(probed[k][0], 'pil')).cuda(non_blocking=True)
    return images, used


def decode_batch_gpu(items, num_workers=8, timings=None, entropy='host', subseq_bytes=0, max_rounds=0):
    """items: file paths or encoded bytes -> (images, used_gpu): a list of CUDA uint8 HxWx3 tensors equal to decode(item, 'pil')
    bit for bit, and a bool per item.  Baseline JPEGs (jpeg_probe) are entropy-decoded on the host by a pool of
    min(num_workers, 16) threads (ctypes releases the GIL) into one pinned buffer, cross the bus in one copy together with their
    tables and descriptors, and are finished by rart_jpeg_decode_u8 in two launches for the whole batch; their images are views
    of one packed buffer.  Every other file (used_gpu False) is decoded by decode(item, 'pil') and uploaded, as the 'pil' reader
    does; what Pillow raises propagates.  timings: a dict that receives 'host_s', 'copy_s', 'device_s' (each phase is then
    followed by a synchronize: a measurement aid).
    entropy='gpu' (opt-in; the default stays 'host'): the file bytes cross the bus instead of the coefficients and
    rart_jpeg_entropy_decode_gpu decodes them, bit-identical to the host decoder (_decode_batch_gpu_entropy; subseq_bytes and
    max_rounds are its parameters, 0 = entropy_params, there 0 = the library's defaults); timings gains 'entropy_s' (launch, status
    read-back and host fallbacks) and 'entropy_kernel_s' (the memset and the kernel, by device events)."""
    global decode_launches
    import ctypes
    import time
    from concurrent.futures import ThreadPoolExecutor
    check_entropy_mode(entropy)
    torch = _lib.require_gpu()
    lib = _lib.load()
    items = list(items)
    n = len(items)
    workers = max(1, min(int(num_workers), MAX_DECODE_WORKERS))
    if entropy == 'gpu':
        return _decode_batch_gpu_entropy(items, workers, timings, int(subseq_bytes) or entropy_params['subseq_bytes'],
                                         int(max_rounds) or entropy_params['max_rounds'])
    t0 = time.perf_counter()

    def probe(item):
        data = _read_bytes(item)
        return data, jpeg_probe(data)

    with ThreadPoolExecutor(max_workers=workers) as pool:
        probed = list(pool.map(probe, items))
        gpu_ids = [k for k in range(n) if probed[k][1].status == 0]
        images, used = [None] * n, [False] * n
        if gpu_ids:
            m = len(gpu_ids)
            descs = (_lib.JpegDesc * m)()
            blk, pix = _fill_jpeg_descs(descs, [probed[k][1] for k in gpu_ids])
            # one staging buffer: descriptors | quantisation tables | coefficients, each region 16-byte aligned
            desc_bytes = (ctypes.sizeof(descs) + 15) // 16 * 16
            qt_bytes = m * 192 * 2
            total = desc_bytes + qt_bytes + blk * 128
            dev = torch.device('cuda', torch.cuda.current_device())
            host, ev = _pinned.pop(dev, (None, None))      # taken out while in use: a concurrent caller stages in a buffer of its own
            if ev is not None:
                ev.synchronize()           # the previous batch's copy has left the buffer
            if host is None or host.numel() < total:
                host = torch.empty(int(total * 1.25), dtype=torch.uint8, pin_memory=True)
            hnp = host.numpy()
            ctypes.memmove(hnp.ctypes.data, ctypes.addressof(descs), ctypes.sizeof(descs))
            qt = hnp[desc_bytes:desc_bytes + qt_bytes].view(np.uint16).reshape(m, 3, 64)
            coef = hnp[desc_bytes + qt_bytes:total].view(np.int16)

            def entropy(j):
                data, info = probed[gpu_ids[j]]
                qt[j] = np.ctypeslib.as_array(info.qt)
                lo = descs[j].block_start[0] * 64
                return jpeg_entropy_decode(data, info, coef[lo:lo + info.coef_count])

            status = list(pool.map(entropy, range(m)))
            if timings is not None:
                timings['host_s'] = time.perf_counter() - t0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            dbuf = torch.empty(total, dtype=torch.uint8, device=dev)
            dbuf.copy_(host[:total], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            _pinned[dev] = (host, ev)
            if timings is not None:
                torch.cuda.synchronize()
                timings['copy_s'] = time.perf_counter() - t0
                t0 = time.perf_counter()
            out = torch.empty(3 * pix, dtype=torch.uint8, device=dev)
            nb = lib.rart_jpeg_decode_workspace_bytes(ctypes.addressof(descs), m)
            ws = _lib.workspace(nb, dev)
            base = dbuf.data_ptr()
            decode_launches += 1
            _lib.check(lib.rart_jpeg_decode_u8(base, ctypes.addressof(descs), m, base + desc_bytes + qt_bytes, blk, base + desc_bytes,
                                               m * 192, _lib.ptr(ws), nb, _lib.ptr(out), out.numel(), _lib.stream_ptr()))
            if timings is not None:
                torch.cuda.synchronize()
                timings['device_s'] = time.perf_counter() - t0
            for j, k in enumerate(gpu_ids):
                if status[j] == 0:         # a stream the entropy decoder gave up on (truncated, corrupt) goes to Pillow below
                    d = descs[j]
                    images[k] = out[d.out_off:d.out_off + 3 * d.height * d.width].view(d.height, d.width, 3)
                    used[k] = True
    for k in range(n):
        if images[k] is None:
            images[k] = torch.from_numpy(decode(probed[k][0], 'pil')).cuda(non_blocking=True)
    return images, used


def _train_params(img_hw, rng):
    """imagenet_s_gen.py:222-263 (random-resized-crop box), with an explicit random.Random."""
    import math
    h, w = img_hw
    area = h * w
    for _ in range(10):
        target_area = rng.uniform(0.08, 1.0) * area
        log_ratio = (math.log(3. / 4.), math.log(4. / 3.))
        ar = math.exp(rng.uniform(*log_ratio))
        cw, chh = int(round(math.sqrt(target_area * ar))), int(round(math.sqrt(target_area / ar)))
        if 0 < cw <= w and 0 < chh <= h:
            return rng.randint(0, h - chh), rng.randint(0, w - cw), chh, cw
    in_ratio = w / h
    if in_ratio < 3. / 4.:
        cw = w
        chh = int(round(cw / (3. / 4.)))
    elif in_ratio > 4. / 3.:
        chh = h
        cw = int(round(chh * (4. / 3.)))
    else:
        cw, chh = w, h
    return (h - chh) // 2, (w - cw) // 2, chh, cw


def image_transfer(image, decoder_type='pil', resize_type='pil-bilinear', transform_type='val', resize=224, seed=None):
    """ImageTransfer(file_path=image, ..., return_online=True).getimage(): (224,224,3) uint8 ndarray.  `image`: a file
    path / encoded bytes, or an already decoded HxWx3 uint8 array."""
    torch = _lib.require_gpu()
    if resize_type not in PIL_FILTERS and resize_type not in CV_MODES:
        raise NotImplementedError(resize_type)
    arr = image if isinstance(image, np.ndarray) else decode(image, decoder_type)
    size = (resize, resize) if not isinstance(resize, tuple) else resize
    is_cv = resize_type in CV_MODES
    op = cv_resize if is_cv else pil_resize
    f = CV_MODES[resize_type] if is_cv else PIL_FILTERS[resize_type]
    if transform_type == 'val':
        first = tuple(int(s * 8 / 7) for s in size)                    # imagenet_s_gen.py:129,139
        th, tw = size
        i, j = int(round((first[0] - th) / 2.)), int(round((first[1] - tw) / 2.))
        dev = torch.from_numpy(np.ascontiguousarray(arr)[None]).cuda()
        return op(dev, first, f, crop=(i, j, th, tw))[0].cpu().numpy()
    if transform_type == 'train':
        # seed None: the GLOBAL random module, like the reference's get_params (imagenet_s_gen.py:222-246), so a user's
        # random.seed(...) makes AddNoise('imagenet-s') reproducible; an explicit seed gets its own generator
        y, x, h, w = _train_params(arr.shape[:2], random if seed is None else random.Random(seed))
        dev = torch.from_numpy(np.ascontiguousarray(arr[y:y + h, x:x + w])[None]).cuda()
        return op(dev, size, f)[0].cpu().numpy()
    raise NotImplementedError(transform_type)


def image_transfer_batch(items, decoder_type='pil', resize_type='pil-bilinear', transform_type='val', resize=224, num_workers=8,
                         decoded=None):
    """The batch form of image_transfer: items (file paths / encoded bytes) -> CUDA uint8 (n, resize, resize, 3), image k equal to
    image_transfer(items[k], ...) (same size rule, same crop offsets; 'train' draws its boxes from the global random module in item
    order).  decoded: the already decoded images (CUDA uint8 HxWx3 tensors, or ndarrays, which are uploaded) -- `items` is then not
    read, so a caller decodes once and resizes many times.  'pil-*' operators run through one pil_resize_batch call, the five
    'opencv-*' operators through one cv_resize_batch call: no per-image call and no copy of a box for either family."""
    torch = _lib.require_gpu()
    if resize_type not in PIL_FILTERS and resize_type not in CV_MODES:
        raise NotImplementedError(resize_type)
    if transform_type not in ('val', 'train'):
        raise NotImplementedError(transform_type)
    if decoder_type != 'pil':
        decode(b'', decoder_type)                  # raises NotImplementedError with decode's message, decoded batch or not
    if decoded is None:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=max(1, min(int(num_workers), MAX_DECODE_WORKERS))) as pool:
            decoded = list(pool.map(lambda it: decode(it, 'pil'), list(items)))
    images = [torch.from_numpy(np.ascontiguousarray(a)).cuda(non_blocking=True) if isinstance(a, np.ndarray) else a for a in decoded]
    size = (resize, resize) if not isinstance(resize, tuple) else resize
    if transform_type == 'val':
        first = tuple(int(s * 8 / 7) for s in size)                    # imagenet_s_gen.py:129,139
        th, tw = size
        crop = (int(round((first[0] - th) / 2.)), int(round((first[1] - tw) / 2.)), th, tw)
        boxes = [None] * len(images)
    else:
        first, crop = size, (0, 0, size[0], size[1])
        boxes = [_train_params(tuple(a.shape[:2]), random) for a in images]
    if resize_type in PIL_FILTERS:
        return pil_resize_batch(images, first, PIL_FILTERS[resize_type], crop=crop, boxes=boxes)
    return cv_resize_batch(images, first, CV_MODES[resize_type], crop=crop, boxes=boxes)
