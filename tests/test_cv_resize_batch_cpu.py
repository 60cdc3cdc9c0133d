"""The batched variable-size OpenCV resize without a device: the host-only plan entry rart_cv_resize_batch_plan (the per-image code
path, the shared tables, the intermediate slots, the documented sizes) and the validation rart_cv_resize_batch_u8 does on the host
copy before any launch."""
import ctypes

import numpy as np

FAKE = 1 << 20            # a non-null, 16-byte aligned "device address": nothing here dereferences it
NEAREST, LINEAR, CUBIC, AREA, LANCZOS4 = 0, 1, 2, 3, 4
FOURTEEN = [(72, 72), (108, 72), (75, 100), (33, 47), (20, 25), (36, 36), (75, 100), (72, 90), (900, 7), (1, 1), (30, 1), (144, 36),
            (37, 35), (72, 72)]
N, T, F, I = 0, 1, 2, 3   # RART_CV_PATH_NEAREST, TWO_PASS, AREA_FLOAT, AREA_INT
# target (36, 36): the rule of oracle/resize_cv_np.resize, image by image
PATHS = {NEAREST: [N] * 14,
         LINEAR: [I] + [T] * 12 + [I],
         CUBIC: [T] * 14,
         LANCZOS4: [T] * 14,
         AREA: [I, I, F, T, T, I, F, F, T, T, T, I, T, I]}


def _descs(sizes, boxes=None):
    from robustart_amd import _lib
    d = (_lib.CvResizeDesc * len(sizes))()
    for k, (h, w) in enumerate(sizes):
        d[k].src, d[k].h, d[k].w = FAKE + 4096 * k, h, w
        d[k].box_y, d[k].box_x, d[k].box_h, d[k].box_w = (boxes[k] if boxes else None) or (0, 0, h, w)
    return d


def _plan(d, interp=LINEAR, target=(36, 36), crop=(2, 2, 32, 32), n=None, fill=True):
    """-> (status, header, host buffer or None)"""
    from robustart_amd import _lib
    lib = _lib.load()
    n = len(d) if n is None else n
    sizes = _lib.CvResizePlan()
    st = lib.rart_cv_resize_batch_plan(ctypes.addressof(d), n, interp, target[0], target[1], *crop, None, 0, ctypes.byref(sizes))
    if st != 0 or not fill:
        return st, sizes, None
    host = np.zeros(sizes.total_bytes, np.uint8)
    short = lib.rart_cv_resize_batch_plan(ctypes.addressof(d), n, interp, target[0], target[1], *crop, host.ctypes.data, host.size - 1,
                                          ctypes.byref(sizes))
    assert short == 3 and not host.any()                       # RART_ERR_WORKSPACE: nothing written, `sizes` says what is needed
    st = lib.rart_cv_resize_batch_plan(ctypes.addressof(d), n, interp, target[0], target[1], *crop, host.ctypes.data, host.size,
                                       ctypes.byref(sizes))
    return st, sizes, host


def _read(host, sizes, n):
    from robustart_amd import _lib
    d = (_lib.CvResizeDesc * n).from_buffer(host, sizes.desc_off)
    prefix = host[sizes.prefix_off:sizes.prefix_off + 8 * (n + 1)].view(np.int64)
    return d, prefix


def test_structs_match_the_documented_layout():
    from robustart_amd import _lib
    assert ctypes.sizeof(_lib.CvResizeDesc) == 64 and ctypes.sizeof(_lib.CvResizePlan) == 80
    assert _lib.CV_PATHS == ('nearest', 'two-pass', 'area-float', 'area-int')
    assert _lib.ABI_VERSION == 110


def test_plan_chooses_the_path_image_by_image():
    for interp, want in PATHS.items():
        st, sizes, host = _plan(_descs(FOURTEEN), interp)
        assert st == 0 and sizes.n == 14 and sizes.interpolation == interp
        d, prefix = _read(host, sizes, 14)
        assert [d[k].path for k in range(14)] == want, interp
        # the intermediate slots cover exactly the two-pass images: mid_count rows of the crop window's 32 columns, int32 samples
        assert prefix[0] == 0
        for k in range(14):
            items = int(prefix[k + 1] - prefix[k])
            if want[k] == T:
                assert 1 <= d[k].mid_count <= d[k].box_h and 0 <= d[k].mid_first <= d[k].box_h - d[k].mid_count
                assert items == d[k].mid_count * 32 * 3, (interp, k)
            else:
                assert items == 0 and (d[k].mid_first, d[k].mid_count) == (0, 0), (interp, k)
        assert sizes.workspace_bytes == (4 * int(prefix[14]) + 255) // 256 * 256
        assert (sizes.workspace_bytes == 0) == (T not in want)
        # integer-area images carry their cell, not a table
        for k in range(14):
            if want[k] == I:
                assert (d[k].ks_y, d[k].ks_x) == (FOURTEEN[k][0] // 36, FOURTEEN[k][1] // 36) and (d[k].tab_x, d[k].tab_y) == (0, 0)
            elif want[k] == T:
                assert d[k].ks_x == d[k].ks_y == {LINEAR: 2, CUBIC: 4, LANCZOS4: 8, AREA: 2}[interp]


def test_plan_shares_tables_between_equal_sizes():
    for interp in PATHS:
        st, sizes, host = _plan(_descs(FOURTEEN), interp)
        assert st == 0
        d, _ = _read(host, sizes, 14)
        # the two (75, 100) images share both tables
        assert (d[2].tab_x, d[2].tab_y, d[2].ks_x, d[2].ks_y) == (d[6].tab_x, d[6].tab_y, d[6].ks_x, d[6].ks_y), interp
        assert d[2].tab_x != d[2].tab_y
        # a table is per (source size, target size, interpolation, axis), not per image: (72, 90) has the rows of (72, 72)
        if d[7].path == d[0].path == T:
            assert d[7].tab_y == d[0].tab_y and d[7].tab_x != d[0].tab_x, interp
        # and a batch that repeats every size needs no more table entries
        st2, twice, _ = _plan(_descs(FOURTEEN + FOURTEEN), interp, fill=False)
        assert st2 == 0 and twice.table_count == sizes.table_count > 0
    # NEAREST: one index table of 36 entries per distinct side; the sides of the fourteen sizes
    st, sizes, host = _plan(_descs(FOURTEEN), NEAREST)
    sides = {s for hw in FOURTEEN for s in hw}
    assert sizes.table_count == 36 * len(sides)
    d, _ = _read(host, sizes, 14)
    tabs = host[sizes.table_off:].view(np.int32)
    assert tabs[d[8].tab_y:d[8].tab_y + 36].tolist() == [25 * y for y in range(36)]              # 900 -> 36
    assert tabs[d[8].tab_x:d[8].tab_x + 36].tolist() == [int(np.floor(x * (1.0 / (36 / 7)))) for x in range(36)]
    assert tabs[d[9].tab_x:d[9].tab_x + 36].tolist() == [0] * 36                                # 1 -> 36


def test_workspace_is_zero_without_a_two_pass_image():
    st, sizes, host = _plan(_descs([(72, 72), (108, 72), (144, 36)]), AREA)
    assert st == 0 and sizes.workspace_bytes == 0 and sizes.table_count == 0
    d, prefix = _read(host, sizes, 3)
    assert [d[k].path for k in range(3)] == [I, I, I] and prefix.tolist() == [0, 0, 0, 0]
    assert [(d[k].ks_y, d[k].ks_x) for k in range(3)] == [(2, 2), (3, 2), (4, 1)]
    st, sizes, _ = _plan(_descs(FOURTEEN), NEAREST, fill=False)
    assert st == 0 and sizes.workspace_bytes == 0
    # a box changes the path of its image: (75, 100) is float-area, its 72 x 72 box integer-area, (108, 72) cut to 100 x 70 float-area
    st, sizes, host = _plan(_descs([(75, 100), (108, 72), (900, 7)], [(1, 2, 72, 72), (3, 0, 100, 70), (100, 2, 800, 2)]), AREA)
    d, prefix = _read(host, sizes, 3)
    assert st == 0 and [d[k].path for k in range(3)] == [I, F, T] and int(prefix[2]) == 0 and int(prefix[3]) == d[2].mid_count * 96


def test_plan_sizes_grow_with_n_as_documented():
    for n in (1, 2, 33):
        st, sizes, _ = _plan(_descs([(33, 47)] * n), CUBIC, fill=False)
        assert st == 0 and sizes.n == n
        assert (sizes.desc_off, sizes.prefix_off) == (80, 80 + 64 * n)
        assert sizes.table_off == sizes.prefix_off + (8 * (n + 1) + 15) // 16 * 16
        assert sizes.total_bytes == sizes.table_off + 4 * sizes.table_count
        assert sizes.table_count == 2 * 36 * (4 + 1)            # 47 -> 36 and 33 -> 36, rows of [first tap, 4 coefficients]: once each
        if n == 1:
            st, one, host = _plan(_descs([(33, 47)]), CUBIC)
            samples = int(_read(host, one, 1)[1][1])
            assert samples > 0
        assert sizes.workspace_bytes == (n * 4 * samples + 255) // 256 * 256     # the int32 intermediates, image after image


def test_plan_refusals_name_what_is_wrong():
    from robustart_amd import _lib
    err = _lib.load().rart_last_error_string
    two = [(33, 47), (75, 100)]
    assert _plan(_descs(two), n=0)[0] == 1 and b'count' in err()
    assert _plan(_descs(two), interp=-1)[0] == 1 and b'interpolation' in err()
    assert _plan(_descs(two), interp=5)[0] == 1 and b'interpolation' in err()
    d = _descs(two)
    d[1].src = 0
    assert _plan(d)[0] == 1 and b'null source' in err()
    assert _plan(_descs([(33, 47), (65536, 2)]))[0] == 1 and b'out of range' in err()
    assert _plan(_descs([(33, 65536), (75, 100)]))[0] == 1 and b'out of range' in err()
    assert _plan(_descs(two, [(0, 0, 34, 47), None]))[0] == 1 and b'box' in err()
    assert _plan(_descs(two, [None, (-1, 0, 75, 100)]))[0] == 1 and b'box' in err()
    assert _plan(_descs(two, [None, (0, 1, 75, 100)]))[0] == 1 and b'box' in err()
    assert _plan(_descs(two, [None, (0, 0, 0, 100)]))[0] == 1 and b'box' in err()
    assert _plan(_descs(two), crop=(2, 5, 32, 32))[0] == 1 and b'crop window' in err()
    assert _plan(_descs(two), crop=(0, 0, 37, 36))[0] == 1 and b'crop window' in err()
    assert _plan(_descs(two), crop=(-1, 0, 36, 36))[0] == 1 and b'crop window' in err()


def test_device_entry_refusals_need_no_device():
    """host copies edited in one field each: every one is refused before any HIP call (the device address is a fake)"""
    from robustart_amd import _lib
    lib = _lib.load()
    err = lib.rart_last_error_string
    # AREA: image 0 two-pass, image 1 float-area, image 2 integer-area
    st, sizes, host = _plan(_descs([(33, 47), (75, 100), (72, 72)]), AREA)
    assert st == 0
    need, out_bytes = int(sizes.workspace_bytes), 3 * 32 * 32 * 3
    assert need > 0

    def call(h=host, ws_bytes=need, out=out_bytes):
        return lib.rart_cv_resize_batch_u8(FAKE, h.ctypes.data, h.size, FAKE, ws_bytes, FAKE, out, None)

    def edited(offset, ctype, value, base=None):
        h = (host if base is None else base).copy()
        ctype.from_buffer(h, offset).value = value
        return h

    i32, P, D = ctypes.c_int32, _lib.CvResizePlan, _lib.CvResizeDesc
    d, prefix = _read(host, sizes, 3)
    assert [d[k].path for k in range(3)] == [T, F, I]
    desc = [sizes.desc_off + 64 * k for k in range(3)]
    assert call(edited(P.n.offset, i32, 0)) == 1 and b'count' in err()
    assert call(edited(P.n.offset, i32, 4)) == 1 and b'region offsets' in err()
    assert call(edited(P.table_off.offset, ctypes.c_int64, sizes.table_off + 16)) == 1 and b'region offsets' in err()
    assert call(edited(P.interpolation.offset, i32, 5)) == 1 and b'interpolation' in err()
    assert call(edited(P.crop_y.offset, i32, 5)) == 1 and b'crop window' in err()
    assert call(edited(desc[0] + D.path.offset, i32, 4)) == 1 and b'path code' in err()
    assert call(edited(desc[1] + D.path.offset, i32, -1)) == 1 and b'path code' in err()
    assert call(edited(desc[2] + D.path.offset, i32, N)) == 1 and b'path code' in err()           # nearest only in a NEAREST call
    assert call(edited(desc[0] + D.box_w.offset, i32, 48)) == 1 and b'box' in err()
    assert call(edited(desc[0] + D.tab_x.offset, i32, int(sizes.table_count) - 8)) == 1 and b'table offset' in err()
    assert call(edited(desc[0] + D.tab_y.offset, i32, -1)) == 1 and b'table offset' in err()
    assert call(edited(desc[1] + D.ks_y.offset, i32, 1 << 15)) == 1 and b'table offset' in err()
    assert call(edited(desc[0] + D.ks_x.offset, i32, 3)) == 1 and b'taps per row' in err()
    # taps: the first row the crop window reads (crop_y = 2) of image 0's vertical table
    row = sizes.table_off + 4 * (d[0].tab_y + 2 * (d[0].ks_y + 1))
    assert call(edited(row, i32, 1 << 21)) == 1 and b'first tap' in err()
    assert call(edited(row, i32, 40)) == 1 and b'taps' in err() and b'outside' in err()            # clamps to row 32, past the range
    assert call(edited(desc[0] + D.mid_first.offset, i32, d[0].mid_first + 1)) == 1 and b'taps' in err()
    # area indices: the first column the crop window reads (crop_x = 2) of image 1's column table [count, (index, alpha) ...]
    row = sizes.table_off + 4 * (d[1].tab_x + 2 * (1 + 2 * d[1].ks_x))
    assert call(edited(row + 4, i32, 100)) == 1 and b'outside the box' in err()
    assert call(edited(row + 4, i32, -1)) == 1 and b'outside the box' in err()
    assert call(edited(row, i32, d[1].ks_x + 1)) == 1 and b'entries' in err()
    assert call(edited(desc[2] + D.ks_x.offset, i32, 3)) == 1 and b'integer-area' in err()         # (2 + 32) * 3 > 72
    assert call(edited(desc[2] + D.ks_y.offset, i32, 0)) == 1 and b'integer-area' in err()
    assert call(edited(desc[0] + D.mid_count.offset, i32, 34)) == 1 and b'intermediate range' in err()
    assert call(edited(desc[0] + D.mid_first.offset, i32, -1)) == 1 and b'intermediate range' in err()
    assert call(edited(sizes.prefix_off, ctypes.c_int64, 3)) == 1 and b'prefix' in err()
    assert call(edited(sizes.prefix_off + 8, ctypes.c_int64, 7)) == 1 and b'prefix' in err()
    assert call(edited(sizes.prefix_off + 16, ctypes.c_int64, int(prefix[2]) + 3)) == 1 and b'prefix' in err()   # float-area: no samples
    assert call(edited(P.workspace_bytes.offset, ctypes.c_int64, 0)) == 1 and b'workspace_bytes' in err()
    assert call(host[:host.size - 4]) == 1 and b'plan_bytes' in err()
    assert call(ws_bytes=need - 1) == 3 and b'workspace' in err()
    assert call(out=out_bytes - 1) == 1 and b'out of' in err()
    assert lib.rart_cv_resize_batch_u8(None, host.ctypes.data, host.size, FAKE, need, FAKE, out_bytes, None) == 1 and b'bad arguments' in err()
    # NEAREST: index tables
    st, sizes, near = _plan(_descs([(33, 47), (900, 7)]), NEAREST)
    assert st == 0 and sizes.workspace_bytes == 0
    d, _ = _read(near, sizes, 2)

    def call_nearest(h):
        return lib.rart_cv_resize_batch_u8(FAKE, h.ctypes.data, h.size, None, 0, FAKE, 2 * 32 * 32 * 3, None)

    entry = sizes.table_off + 4 * (d[1].tab_x + 2)
    assert call_nearest(edited(entry, i32, 7, near)) == 1 and b'table entry' in err()
    assert call_nearest(edited(entry, i32, -1, near)) == 1 and b'table entry' in err()
    assert call_nearest(edited(sizes.desc_off + D.path.offset, i32, T, near)) == 1 and b'path code' in err()
    assert call_nearest(edited(sizes.desc_off + 64 + D.tab_y.offset, i32, int(sizes.table_count) - 35, near)) == 1 and b'table offset' in err()
