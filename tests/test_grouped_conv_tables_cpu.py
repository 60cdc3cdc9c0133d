"""`_Conv` of a grouped 3x3 on the CPU: the slice tables, multiplied out in fp64 under the launch semantics of rart_conv3x3_grouped_*,
equal F.conv2d(groups = G) and torch.nn.grad.conv2d_input exactly on integer-valued operands (forward, backward at stride 1, the four
input-parity classes at stride 2); off-block entries are exact zeros; the fragment-ordered copy holds the same values; the hi + lo planes
of the pair form sum to the folded fp32 weight within 2^-16; and the operands of tests/test_grouped_conv_gpu.py make both wrong
references (groups shifted, groups ignored) violate that test's bounds in at least 90 % of the outputs."""
import pytest
import torch
import torch.nn.functional as F

import _grouped_conv_ref as R

WIDTHS = [(64, 4), (64, 8), (64, 16), (64, 32), (128, 64)]


def _int_conv(C, gw, stride, seed):
    g = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv2d(C, C, 3, stride=stride, padding=1, groups=C // gw, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randint(-4, 5, conv.weight.shape, generator=g).float())
    return conv


def _conv(conv, bn, split):
    from robustart_amd.model.engine import _Conv
    return _Conv(conv, bn, 'cpu', split)


@pytest.mark.parametrize('split', [False, True])
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('C,gw', WIDTHS)
def test_slice_tables_multiply_out_to_the_grouped_convolution(C, gw, stride, split):
    conv = _int_conv(C, gw, stride, 7 * C + gw + stride)
    c = _conv(conv, None, split)
    S, G = c.slice, C // gw
    assert (c.groups, c.gw, c.cin, c.cout, S) == (G, gw, C, C, 64 if gw == 64 else 32)
    assert c.w_fwd is None and all(t is None for _, _, t in c.bwd)            # no dense table exists
    g = torch.Generator().manual_seed(3)
    h, w = 6, 8
    x = torch.randint(-3, 4, (2, C, h, w), generator=g).double()
    wd = conv.weight.detach().double()
    oh, ow = h // stride, w // stride
    got = R.apply_tables(R.table_planes(c.g_fwd[0], 9 * S, split), S, c.fwd_taps, x, (oh, ow), stride)
    assert torch.equal(got, F.conv2d(x, wd, None, stride, 1, 1, G))
    dz = torch.randint(-3, 4, (2, C, oh, ow), generator=g).double()
    want = torch.nn.grad.conv2d_input(x.shape, wd, dz, stride, 1, 1, G)
    assert len(c.g_bwd) == (1 if stride == 1 else 4)
    dx = torch.full_like(want, 77.0)
    for (parity, taps, _), (rows, _) in zip(c.bwd, c.g_bwd):
        assert len(taps) == (9 if stride == 1 else {(0, 0): 1, (0, 1): 2, (1, 0): 2, (1, 1): 4}[parity])
        tab = R.table_planes(rows, len(taps) * S, split)
        if parity is None:
            dx = R.apply_tables(tab, S, taps, dz, (h, w))
        else:
            part = R.apply_tables(tab, S, taps, dz, (h // 2, w // 2), 1, (h, w), 2, parity, fill=77.0)
            written = torch.zeros(h, w, dtype=torch.bool)
            written[parity[0]::2, parity[1]::2] = True
            assert (part[:, :, ~written] == 77.0).all()                        # a class writes its parity alone
            dx[:, :, written] = part[:, :, written]
    assert torch.equal(dx, want)


@pytest.mark.parametrize('split', [False, True])
@pytest.mark.parametrize('C,gw', WIDTHS)
def test_off_block_entries_are_exact_zeros_and_the_fragment_copy_holds_the_same_values(C, gw, split):
    conv, bn = R.make_layer(C, gw, 2)
    c = _conv(conv, bn, split)
    S, ns = c.slice, C // c.slice
    same_group = (torch.arange(S).view(-1, 1) // gw) == (torch.arange(S).view(1, -1) // gw)
    for rows, frag in [c.g_fwd] + list(c.g_bwd):
        k = rows.shape[2] // (3 if split else 1)
        assert rows.shape[:2] == (ns, 64) and rows.dtype == torch.bfloat16 and k % (S) == 0
        planes = [rows[:, :, i * k:(i + 1) * k] for i in range(3 if split else 1)]
        if split:
            assert torch.equal(planes[0], planes[2])                           # [hi | lo | hi]
        for p in planes:
            assert (p[:, S:] == 0).all()                                       # rows that pad the GEMM tile
            blocks = p[:, :S].reshape(ns, S, k // S, S)
            assert (blocks[:, ~same_group.view(S, 1, S).expand(S, k // S, S)] == 0).all()
            assert (blocks != 0).float().mean().item() > 0.9 * gw / S          # ... and the block diagonal is populated
        fr = frag if split else frag.unsqueeze(0)
        for i in range(fr.shape[0]):
            assert torch.equal(R.frag_decode(fr[i], ns, S, k), planes[i][:, :S])


@pytest.mark.parametrize('C,gw', WIDTHS)
def test_pair_planes_sum_to_the_folded_weight(C, gw):
    conv, bn = R.make_layer(C, gw, 1)
    c = _conv(conv, bn, True)
    S, G = c.slice, C // gw
    inv = (bn.running_var + bn.eps).rsqrt() * bn.weight
    wf = (conv.weight * inv.view(-1, 1, 1, 1)).detach()
    assert torch.equal(c.w_folded, wf)
    assert torch.allclose(c.b_folded, (bn.bias - bn.running_mean * inv).detach(), rtol=0, atol=1e-7)
    tab = R.table_planes(c.g_fwd[0], 9 * S, True)[:, :S].reshape(C // S, S, 9, S)       # [slice][o][tap][c]
    for o in range(0, C, 7):
        i, ol = divmod(o, S)
        g0 = (ol // gw) * gw                                                   # first slice-local input channel of o's group
        got = tab[i, ol, :, g0:g0 + gw].t().reshape(gw, 3, 3)
        want = wf[o].double()
        assert ((got - want).abs() <= want.abs() * 2.0 ** -16).all()


@pytest.mark.parametrize('split', [False, True])
@pytest.mark.parametrize('C,gw', R.CASES)
def test_wrong_references_violate_the_gpu_tests_bounds_in_nine_outputs_of_ten(C, gw, split):
    """the operands of tests/test_grouped_conv_gpu.py: a result computed with every group's weights moved to the next group, or with
    `groups` ignored, misses the bound nearly everywhere -- so a kernel that passes there has the group structure right"""
    viol = R.pair_violations if split else R.bf16_violations
    G = C // gw
    # the GPU test's size list; its third stride-1 size is (tile rows + 3) x (16 + 5) from the library's query: tiles of 16 or 8 rows
    for stride, hw in ((1, (5, 7)), (1, (14, 14)), (1, (19, 21)), (1, (11, 21)), (2, (8, 12)), (2, (14, 14))):
        conv, bn = R.make_layer(C, gw, stride)
        c = _conv(conv, bn, split)
        w, b = R.stored(c.w_folded, split), c.b_folded.double()
        x, _ = R.inputs(C, hw, 11)
        xs = R.stored(x, split)
        ref = R.ref_forward(xs, w, b, stride, G)
        share = [viol(R.ref_forward(xs, R.shifted(w, gw), b, stride, G), ref).float().mean().item(),
                 viol(R.ref_forward(xs, R.dense_weight(w, G), b, stride, 1), ref).float().mean().item()]
        oh, ow = hw[0] // stride, hw[1] // stride
        dz, _ = R.inputs(C, (oh, ow), 12)
        _, mask = R.inputs(C, hw, 13)
        dzs = R.stored(dz, split)
        refb = R.ref_backward(dzs, w, hw, stride, G, mask)
        share += [viol(R.ref_backward(dzs, R.shifted(w, gw), hw, stride, G, mask), refb).float().mean().item(),
                  viol(R.ref_backward(dzs, R.dense_weight(w, G), hw, stride, 1, mask), refb).float().mean().item()]
        print('C %d gw %d stride %d %dx%d %s: wrong-reference violation shares fwd shifted %.3f dense %.3f, bwd shifted %.3f dense %.3f'
              % ((C, gw, stride, hw[0], hw[1], 'pair' if split else 'bf16') + tuple(share)))
        assert min(share) >= 0.9, share
        assert (ref > 0).float().mean().item() < 0.99                          # the ReLU still clamps
