"""GPU: the pose encoder in HIP (include/dragposer_encoder.h: dp_encode, dp_sequence_begin; dragposer_amd.NativePoseEncoder;
DragPose(native_encoder=True)) against the real reference (tests/golden/enc.npz) and the fp64 PyTorch encoder.

Tolerance: the project's own for the encoder (tests/test_host_pipeline.py): mu, logvar atol 2e-5 rtol 1e-5; latent atol 5e-5 rtol 1e-5.
On the CPU the NumPy emulation of the kernel's arithmetic (tests/encoder_emu.py) is within 24 % of that bar on the golden poses (4.8e-6 on
logvar) and 29 % on the 1017 normal poses used here (5.8e-6 on logvar)."""
import os

import numpy as np
import pytest
import torch

from dragposer_amd import _lib
from dragposer_amd.encoder import NativePoseEncoder, PoseEncoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MU_TOL = dict(atol=2e-5, rtol=1e-5)
LATENT_TOL = dict(atol=5e-5, rtol=1e-5)
BAD = _lib.DP_STATUS_BAD_STATE | _lib.DP_STATUS_NONFINITE_RESULT
SIZES = (1, 15, 16, 17, 33, 1000)


@pytest.fixture(scope="module")
def enc():
    return NativePoseEncoder(device=DEV)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "enc.npz"))


@pytest.fixture(scope="module")
def poses():
    """1000 + 17 standard-normal poses and their eps (never modified)"""
    g = torch.Generator().manual_seed(7)
    return torch.randn(1017, 176, generator=g), torch.randn(1017, 24, generator=g)


@pytest.fixture(scope="module")
def ref64(poses):
    """the fp64 PyTorch encoder on the CPU, once for every test that needs it"""
    with torch.no_grad():
        mu, lv = PoseEncoder().double()(poses[0].double())
    return mu.numpy(), lv.numpy()


@pytest.fixture(scope="module")
def big(enc, poses):
    """the 1000-pose launch, once: the bits every position-independence check compares with"""
    o = enc.encode(poses[0][:1000].to(DEV), eps=poses[1][:1000].to(DEV))
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in o.items()}


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def test_reference_parity_on_the_golden_poses(enc, golden):
    o = enc.encode(torch.tensor(golden["pose"]), eps=torch.tensor(golden["eps"]))  # 24 poses: a full tile and a ragged one
    np.testing.assert_allclose(o["mu"].cpu().numpy(), golden["mu"], **MU_TOL)
    np.testing.assert_allclose(o["logvar"].cpu().numpy(), golden["logvar"], **MU_TOL)
    np.testing.assert_allclose(o["latent"].cpu().numpy(), golden["latent"], **LATENT_TOL)
    assert not o["status"].any()
    mu, lv = enc(torch.tensor(golden["pose"]))  # PoseEncoder's interface
    assert torch.equal(mu, o["mu"]) and torch.equal(lv, o["logvar"])
    z = enc.sample(torch.tensor(golden["pose"]), generator=torch.Generator().manual_seed(3))
    eps = torch.randn(24, 24, generator=torch.Generator().manual_seed(3))
    assert torch.equal(z, enc.encode(torch.tensor(golden["pose"]), eps=eps)["latent"])
    assert torch.equal(enc.sample(torch.tensor(golden["pose"]), use_mean=True), o["mu"])


@pytest.mark.parametrize("B", SIZES)
def test_ragged_sizes_against_the_fp64_encoder(enc, poses, ref64, B):
    o = enc.encode(poses[0][:B].to(DEV))
    err_mu = np.abs(o["mu"].cpu().numpy() - ref64[0][:B]).max()
    err_lv = np.abs(o["logvar"].cpu().numpy() - ref64[1][:B]).max()
    print(f"B={B}: max |mu - fp64| {err_mu:.3e}, max |logvar - fp64| {err_lv:.3e}")
    np.testing.assert_allclose(o["mu"].cpu().numpy(), ref64[0][:B], **MU_TOL)
    np.testing.assert_allclose(o["logvar"].cpu().numpy(), ref64[1][:B], **MU_TOL)
    assert torch.equal(o["latent"], o["mu"]) and not o["status"].any()


def test_a_pose_has_the_same_bits_wherever_it_stands(enc, poses, big):
    x, e = poses[0].to(DEV), poses[1].to(DEV)
    for i in (0, 15, 16, 500, 999):
        alone = enc.encode(x[i:i + 1], eps=e[i:i + 1])
        batch_x, batch_e = x[1000:1017].clone(), e[1000:1017].clone()
        j = (i * 7 + 3) % 17
        batch_x[j], batch_e[j] = x[i], e[i]
        moved = enc.encode(batch_x, eps=batch_e)
        for k in ("mu", "logvar", "latent"):
            assert np.array_equal(_bits(alone[k][0]), _bits(big[k][i])), (i, k)
            assert np.array_equal(_bits(moved[k][j]), _bits(big[k][i])), (i, j, k)


def test_second_trip_of_the_persistent_loop(enc, poses, ref64, big):
    ppw, wpb, blocks = enc.geometry()
    assert ppw == 16 and wpb >= 1 and blocks >= 1
    B = ppw * wpb * blocks + 17
    x = torch.zeros(B, 176, device=DEV)
    e = torch.zeros(B, 24, device=DEV)
    x[:1000], e[:1000] = poses[0][:1000].to(DEV), poses[1][:1000].to(DEV)
    x[-17:], e[-17:] = poses[0][1000:].to(DEV), poses[1][1000:].to(DEV)
    o = enc.encode(x, eps=e)
    for k in ("mu", "logvar", "latent"):
        assert np.array_equal(_bits(o[k][:1000]), _bits(big[k])), k
    np.testing.assert_allclose(o["mu"][-17:].cpu().numpy(), ref64[0][1000:], **MU_TOL)
    np.testing.assert_allclose(o["logvar"][-17:].cpu().numpy(), ref64[1][1000:], **MU_TOL)
    with torch.no_grad():
        mu, lv = ref64[0][1000:], ref64[1][1000:]
        z = mu + poses[1][1000:].double().numpy() * np.exp(0.5 * lv)
    np.testing.assert_allclose(o["latent"][-17:].cpu().numpy(), z, **LATENT_TOL)
    assert not o["status"].any()


def test_eps_null_and_zero_and_optional_outputs(enc, poses, big):
    x = poses[0][:33].to(DEV)
    none = enc.encode(x)
    zero = enc.encode(x, eps=torch.zeros(33, 24, device=DEV))
    assert np.array_equal(_bits(none["latent"]), _bits(none["mu"]))
    assert np.array_equal(_bits(zero["latent"]), _bits(zero["mu"])) and np.array_equal(_bits(zero["mu"]), _bits(big["mu"][:33]))
    e = poses[1][:33].to(DEV)
    for keep in (("mu",), ("logvar",), ("latent",), ("status",), ("mu", "latent")):
        o = enc.encode(x, eps=e, outputs=keep)  # the others are NULL
        assert set(o) == set(keep)
        for k in keep:
            assert np.array_equal(o[k].cpu().numpy().view(np.uint32), big[k][:33].cpu().numpy().view(np.uint32)), (keep, k)
    empty = enc.encode(torch.zeros(0, 176, device=DEV))  # n == 0: nothing is launched
    assert empty["mu"].shape == (0, 24)


def test_screening_refuses_a_pose_and_leaves_its_neighbours_alone(enc, poses):
    x, e = poses[0][:48].to(DEV).clone(), poses[1][:48].to(DEV).clone()
    clean = enc.encode(x, eps=e)
    x[5, 100] = float("nan")
    e[20, 3] = float("inf")
    x[37, 0] = 1e9
    o = enc.encode(x, eps=e)
    badrows = [5, 20, 37]
    good = [i for i in range(48) if i not in badrows]
    for k in ("mu", "logvar", "latent"):
        assert torch.isnan(o[k][badrows]).all(), k
        assert np.array_equal(_bits(o[k][good]), _bits(clean[k][good])), k
    assert o["status"][badrows].tolist() == [BAD] * 3 and not o["status"][good].any() and not clean["status"].any()


def _begin_inputs(poses, S, NH):
    g = torch.Generator().manual_seed(11)
    pos, rot, hts = torch.randn(S, 3, generator=g), torch.randn(S, 4, generator=g), torch.rand(S, NH, generator=g)
    return poses[0][:S].to(DEV), poses[1][:S].to(DEV), pos.to(DEV), rot.to(DEV), hts.to(DEV)


def _begin(enc, x, e, pos, rot, hts, H):
    """dp_sequence_begin into state tensors pre-filled with NaN"""
    import ctypes as C

    S, NH = x.shape[0], hts.shape[1]
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    o = dict(latent=nan(S, 24), global_pos=nan(S, 3), global_rot=nan(S, 4), latent_buf=nan(S, H, 24), disp_buf=nan(S, H, 3),
             heights_buf=nan(S, H, NH), status=torch.full((S,), -1, dtype=torch.int32, device=DEV))
    st = _lib.DpSeqState()
    st.global_pos, st.global_rot, st.latent_buf = o["global_pos"].data_ptr(), o["global_rot"].data_ptr(), o["latent_buf"].data_ptr()
    st.disp_buf, st.heights_buf, st.history, st.n_heights = o["disp_buf"].data_ptr(), o["heights_buf"].data_ptr(), H, NH
    rc = enc._lib.dp_sequence_begin(enc._h, S, x.data_ptr(), e.data_ptr(), pos.data_ptr(), rot.data_ptr(), hts.data_ptr(), C.byref(st),
                                    o["latent"].data_ptr(), o["status"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, enc._lib.dp_encoder_last_error(enc._h)
    torch.cuda.synchronize()
    return o


def test_sequence_begin_writes_every_element_of_the_state(enc, poses, big):
    S, H, NH = 5, 60, 6
    x, e, pos, rot, hts = _begin_inputs(poses, S, NH)
    o = _begin(enc, x, e, pos, rot, hts, H)
    assert np.array_equal(_bits(o["latent"]), _bits(big["latent"][:S]))
    assert np.array_equal(_bits(o["latent_buf"]), _bits(o["latent"].unsqueeze(1).expand(S, H, 24).contiguous()))
    assert (o["disp_buf"] == 0).all()
    assert torch.equal(o["heights_buf"], hts.unsqueeze(1).expand(S, H, NH))
    assert torch.equal(o["global_pos"], pos) and torch.equal(o["global_rot"], rot)
    assert all(torch.isfinite(v).all() for k, v in o.items() if k != "status") and not o["status"].any()
    # a NaN in one sequence's initial rotation refuses that sequence alone
    rot2 = rot.clone()
    rot2[3, 2] = float("nan")
    p = _begin(enc, x, e, pos, rot2, hts, H)
    others = [0, 1, 2, 4]
    for k in ("latent", "global_pos", "global_rot", "latent_buf", "disp_buf", "heights_buf"):
        assert torch.isnan(p[k][3]).all(), k
        assert np.array_equal(_bits(p[k][others]), _bits(o[k][others])), k
    assert p["status"].tolist() == [0, 0, 0, BAD, 0]
    # NativePoseEncoder.begin allocates the same state
    q = enc.begin(x, e, pos, rot, hts, H)
    for k in o:
        assert torch.equal(q[k], o[k]), k


def test_dragpose_with_the_native_encoder(golden):
    from dragposer_amd.drag_pose import DragPose
    from oracle import ref_torch as R

    S = len(golden["pose"])
    rot = np.tile(np.array([1, 0, 0, 0], np.float32), (S, 1))
    gpos = np.arange(3 * S, dtype=np.float32).reshape(S, 3, 1) * 0.01
    args = (golden["pose"].reshape(S, 176, 1), gpos, rot.reshape(S, 4, 1), np.tile(golden["heights"], (S, 1)))
    default = DragPose(None, None, np.zeros(24), np.ones(24), "cpu", DEV, n_sequences=S)
    native = DragPose(default.opt, None, np.zeros(24), np.ones(24), "cpu", DEV, n_sequences=S, native_encoder=True)
    default.set_initial_pose(*args, eps=golden["eps"])
    native.set_initial_pose(*args, eps=golden["eps"])
    np.testing.assert_allclose(native.latent.cpu().numpy(), golden["latent"], **LATENT_TOL)
    np.testing.assert_allclose(native.latent.cpu().numpy(), default.latent.cpu().numpy(), **LATENT_TOL)
    np.testing.assert_allclose(native.latent_buffer.cpu().numpy(), default.latent_buffer.cpu().numpy(), **LATENT_TOL)
    for name in ("current_global_pos", "current_global_rot", "displacement_buffer", "heights_buffer"):
        assert torch.equal(getattr(native, name), getattr(default, name)), name
    assert native.current_index == 0 and native.target_latent_buffer is None and not native.begin_status.any()
    # one frame from it, as tests/test_hip_sequences.py::test_reference_constructor_and_set_initial_pose runs it
    one = DragPose(default.opt, None, np.zeros(24), np.ones(24), "cpu", DEV, native_encoder=True)
    one.set_initial_pose(golden["pose"][3].reshape(1, 176, 1), np.zeros((1, 3, 1), np.float32), np.array([1, 0, 0, 0], np.float32).reshape(1, 4, 1),
                         golden["heights"], eps=golden["eps"][3])
    np.testing.assert_allclose(one.latent.cpu().numpy()[0], golden["latent"][3], **LATENT_TOL)
    b = R.synth_inputs(R.OracleModel(), 1)
    idx = np.array(R.TRACK6)
    pose, pos = one.run(torch.tensor(b["tgt_pos"][0, idx]), torch.tensor(b["tgt_rot"][0, idx]).reshape(6, 3, 3), idx,
                        np.array([R.W6[j] for j in R.TRACK6], np.float32), max_iter=10, learning_rate=1e-2, lambda_temporal=0.0,
                        temporal_future_window=0)
    assert tuple(pose.shape) == (88,) and torch.isfinite(pose).all() and torch.isfinite(pos).all()


def test_encode_is_capturable_into_a_graph(enc, poses, big):
    x, e = poses[0][:33].to(DEV), poses[1][:33].to(DEV)
    out = {k: torch.empty_like(big[k][:33]) for k in ("mu", "logvar", "latent", "status")}
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        enc.encode(x, eps=e, out=out)  # (a first launch outside the capture)
    torch.cuda.current_stream(DEV).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream, one kernel node: no parallel branch
        enc.encode(x, eps=e, out=out)
    for _ in range(2):
        for v in out.values():
            v.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        for k in out:
            assert torch.equal(out[k], big[k][:33]), k
