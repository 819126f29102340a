"""CPU: the float64 references of tests/train_aux_refs.py against float64 torch autograd of the reference project's own operations (1e-12 relative, every
case of the GPU module), the margins the input builders promise (no pre-activation within 1e-3 of zero; ambiguous max-pool windows <= 0.1 %), and
soccdpt_op_train_aux_scratch_bytes on every case: a non-zero size inside the GPU module's scratch buffer for the good ones, 0 and an error for the
refused ones.  That entry launches nothing, so no GPU is needed."""
import ctypes

import pytest
import torch

from tests import train_aux_refs as R

TOL = 1e-12
D = torch.float64


def _close(ref, other, names, what):
    for n in names:
        err = R.rel_l2(other[n], ref[n])
        assert err < TOL, f"{what}: {n} differs from torch float64 autograd by {err:.2e}"


@pytest.mark.parametrize("case", list(R.LN_CASES))
def test_layer_norm_reference(case):
    inp = R.build_ln(case)
    _close(R.ref_ln(inp), R.torch_ln(inp), ("dy", "xhat", "dgamma", "dbeta"), case)


@pytest.mark.parametrize("case", list(R.BN_CASES))
def test_batch_norm_reference_and_margin(case):
    inp = R.build_bn(case)
    assert float(inp["pre64"].abs().min()) > R.MARGIN
    assert 0.05 < float((inp["pre64"] > 0).float().mean()) < 0.95           # the mask is not trivial
    _close(R.ref_bn(inp), R.torch_bn(inp), ("stats", "rmean", "rvar", "y", "dbeta", "dgamma", "dx"), case)


@pytest.mark.parametrize("case", list(R.GN_CASES))
def test_group_norm_reference_and_margin(case):
    inp = R.build_gn(case)
    if inp["relu"]:
        assert float(inp["pre64"].abs().min()) > R.MARGIN
        assert 0.05 < float((inp["pre64"] > 0).float().mean()) < 0.95
    _close(R.ref_gn(inp), R.torch_gn(inp), ("dx", "dgamma", "dbeta"), case)
    # the statistics handed to the kernel are the float64 ones, rounded
    B, HW, C = inp["x"].shape
    assert inp["stats"].shape == (B, C // inp["cpg"], 2) and inp["stats"].dtype == torch.float32


@pytest.mark.parametrize("case", list(R.WS_CASES))
def test_weight_standardisation_reference(case):
    inp = R.build_ws(case)
    _close(R.ref_ws(inp), R.torch_ws(inp), ("dw",), case)
    Cout, Cin, k, Kpad = R.WS_CASES[case]
    fan = Cin * k * k
    assert inp["dwh"].shape == inp["wh"].shape == (Cout, Kpad)
    assert bool(torch.isnan(inp["dwh"][:, fan:]).all()) and bool(torch.isfinite(inp["dwh"][:, :fan]).all())
    # tap-major: column tap * Cin + ci holds the parameter's [ci][ky][kx]
    assert torch.equal(inp["dwh"][:, :fan].reshape(Cout, k, k, Cin).permute(0, 3, 1, 2), inp["dwh_param"])


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", R.BILINEAR_SHAPES, ids=str)
def test_bilinear_reference(shape, accumulate):
    inp = R.build_bilinear(shape, accumulate)
    _close(R.ref_bilinear(inp), R.torch_bilinear(inp), ("dlo",), shape)


@pytest.mark.parametrize("shape", R.MAXPOOL_SHAPES, ids=str)
def test_max_pool_reference_and_ambiguous_share(shape):
    inp = R.build_maxpool(shape)
    ref = R.ref_maxpool(inp)
    _close(ref, R.torch_maxpool(inp), ("dA",), shape)
    win = R._pool_windows(R.pool_activation(inp))
    first, decided, wmax = R.pool_classes(win)
    assert float((~decided).float().mean()) <= R.POOL_AMBIGUOUS_SHARE
    # torch's own choice (return_indices over the padded image) is the first maximum in scan order
    B, Hi, C, _ = shape
    A = R.pool_activation(inp).permute(0, 3, 1, 2)
    _, flat = torch.nn.functional.max_pool2d(R.pad_same(A, 3, 2, value=float("-inf")), 3, 2, return_indices=True)
    oy = torch.arange(Hi // 2).view(1, 1, -1, 1)
    ox = torch.arange(Hi // 2).view(1, 1, 1, -1)
    tap = (flat // (Hi + 1) - 2 * oy) * 3 + (flat % (Hi + 1) - 2 * ox)
    assert torch.equal(tap.permute(0, 2, 3, 1), first.long())
    assert bool((ref["idx"] < 9).all())
    # some windows are all zero, some reach the padding
    assert bool((wmax == 0).any()) and bool(torch.isinf(win).any())


@pytest.mark.parametrize("shape", R.DEPTH_TAIL_SHAPES, ids=str)
def test_depth_tail_reference_and_margin(shape):
    inp = R.build_depth_tail(shape)
    K, M = shape
    assert inp["e"].shape == (M, K)
    assert float(inp["s64"].abs().min()) > R.MARGIN and float(inp["e"].abs().min()) > R.MARGIN
    if M > 30:
        assert 0.05 < float((inp["s64"] > 0).float().mean()) < 0.95
    ref, t = R.ref_depth_tail(inp), R.torch_depth_tail(inp)
    _close(ref, t, ("inv", "de"), shape)
    assert R.rel_l2(ref["rowterm"][:, :K].sum(0), t["dw4"]) < TOL and R.rel_l2(ref["rowterm"][:, K].sum(0, keepdim=True), t["db4"]) < TOL


@pytest.mark.parametrize("shape", R.SMALLK_SHAPES, ids=str)
def test_smallk_reference(shape):
    inp = R.build_smallk(shape)
    _close(R.ref_smallk(inp), R.torch_smallk(inp), ("dx", "dw"), shape)


def test_elementwise_references():
    inp = R.build_gelu()
    _close(R.ref_gelu(inp), R.torch_gelu(inp), ("dx",), "gelu")
    for with_add in (False, True):
        for halo in (None, (2, 5, 7, 12)):
            inp = R.build_relu(with_add, halo)
            assert bool((inp["ref"] == 0).any())
            _close(R.ref_relu(inp), R.torch_relu(inp), ("dx",), "relu")
    for sigmoid in (0, 1):
        inp = R.build_seg_act(sigmoid)
        err = R.rel_l2(R.torch_seg_act(inp)["dup"], R.ref_seg_act(inp)["dup"])
        assert err < 1e-9, err            # through logit(): the saved f32 output's inverse costs a few digits
    inp = R.build_merge_scatter()
    assert torch.equal(R.ref_merge_scatter(inp)["dx"].double(), R.torch_merge_scatter(inp)["dx"])
    inp = R.build_scale_rows()
    M, C, rps = inp["shape"]
    out = R.ref_scale_rows(inp)["out"]
    assert out.dtype == torch.float32 and torch.equal(out[rps:2 * rps], inp["in"][rps:2 * rps] * inp["scale"][1]) and bool((out[:rps] == 0).all())


def test_colsum_reference_is_the_definition():
    inp = R.build_colsum((17, 65), True, 1, False)
    ref = R.ref_colsum(inp)
    a, b = inp["a"].double(), inp["b"].double()
    want = torch.stack([sum(a[m, n] * b[m, n] for m in range(17)) for n in range(65)])
    assert R.rel_l2(ref["out_ab"], want) < TOL and R.rel_l2(ref["out"], want + inp["out0"].double()) < TOL
    assert R.rel_l2(ref["out_a"], a.sum(0)) < TOL


# ---------------- the scratch sizes, without a GPU ----------------
def _args(spec):
    """TrainAuxArgs for a Spec with a placeholder in every pointer the spec names (soccdpt_op_train_aux_scratch_bytes dereferences none)."""
    from tests import test_train_aux_gpu as G
    return G.make_args(spec, ptr=1 << 20)


def test_scratch_bytes_of_every_case():
    from soccdpt_amd.lib import load_library, op_train_aux_scratch_bytes
    from tests import test_train_aux_gpu as G
    L = load_library()
    specs = G.all_specs()
    assert len(specs) > 100 and {s.kind for _, s in specs} == set(R.KINDS)
    for label, spec in specs:
        need = op_train_aux_scratch_bytes(_args(spec))
        assert 0 < need <= G.SCRATCH_BYTES and need % 256 == 0, (label, need)
    # the sizes are the launchers' own: chunks * N (colsum), chunks * 2N (colsum2, LayerNorm), (128 C + C) doubles (bn_stats),
    # B chunks 2C + B G 2 (gn_bwd), 256 K C (smallk_wgrad)
    up = lambda floats: max(256, (4 * floats + 255) // 256 * 256)

    def colsum_chunks(M, N):
        return max(1, min(512 // ((N + 63) // 64), (M + 15) // 16))

    def gn_chunks(B, HW, C):
        return max(1, min(512 // (((C + 63) // 64) * B), (HW + 15) // 16))
    for M, N in R.COLSUM_SHAPES:
        assert op_train_aux_scratch_bytes(_args(R.spec_colsum((M, N), True, 0, False))) == up(colsum_chunks(M, N) * N)
        assert op_train_aux_scratch_bytes(_args(R.spec_colsum((M, N), True, 0, True))) == up(colsum_chunks(M, N) * 2 * N)
    assert colsum_chunks(4099, 288) == 102 and colsum_chunks(2063, 2304) == 14 and colsum_chunks(1, 64) == 1
    for case, (M, C, _, _) in R.LN_CASES.items():
        assert op_train_aux_scratch_bytes(_args(R.spec_ln(case))) == up(colsum_chunks(M, C) * 2 * C)
    for case, (M, C, _, _) in R.BN_CASES.items():
        assert op_train_aux_scratch_bytes(_args(R.spec_bn_fwd(case))) == up(2 * (128 * C + C))
    for case, ((B, HW, C, cpg, _), _) in R.GN_CASES.items():
        assert op_train_aux_scratch_bytes(_args(R.spec_gn(case))) == up(B * gn_chunks(B, HW, C) * 2 * C + B * (C // cpg) * 2)
    assert gn_chunks(40, 4, 1024) == 1 and 512 // (16 * 40) == 0
    for M, C, K in R.SMALLK_SHAPES:
        assert op_train_aux_scratch_bytes(_args(R.spec_smallk((M, C, K)))) == up(256 * K * C)
    # refused: 0 and a message
    for label, a in G.bad_args(_args):
        assert L.soccdpt_op_train_aux_scratch_bytes(ctypes.byref(a)) == 0, label
        assert L.soccdpt_last_error(None).decode().startswith("soccdpt_op_train_aux"), label
        with pytest.raises(RuntimeError):
            op_train_aux_scratch_bytes(a)
    assert L.soccdpt_op_train_aux_scratch_bytes(None) == 0
