"""The fused MLP over its whole descriptor range on an MI355X (``-m gpu``).

``mlp_check_desc`` (csrc/mlp_pack.hip) takes n_blocks 1..8, any combine_layer >= 0 and pe_n
0..16; every other GPU test runs n_blocks = 5, combine_layer = 3, num_freqs = 6.  The
descriptors here are written (n_blocks, combine_layer, num_freqs, NS source views), with
d_in = 6 + 6 num_freqs; weights from ``synth.pixelnerf_state``, the oracle is
``ref_cpu.pixelnerf_forward(.., n_blocks=, combine_layer=)``.

Tolerances are the project's own (tests/test_gpu_parity.py: |hip - ref| <= 5e-5 + 1e-5 |ref|;
tests/test_gpu_f16.py: bounded by the emulation).  The fp32 oracle's own distance to an fp64
oracle is at most 0.17 of that tolerance on these models (the two 8-block single-view ones;
0.09 elsewhere), as on the shipped 5 / 3 model (0.08): the kernel keeps about 5 x the
reference's rounding.

Order: the host refusals (no launch) and the fp32 point queries first.
"""
import functools

import pytest
import torch

import test_gpu_parity as tgp
from oracle import ref_cpu
from pnr import _lib, synth, util
from pnr.models import PixelNeRFNet
from pnr.renderer import DotMap, NeRFRenderer
from test_gpu_f16 import bounded_raw, with_emulation

pytestmark = pytest.mark.gpu
DEV = tgp.DEV

DESCS = {
    1: (3, 1000, 6, 1),    # the reference's conf/default.conf: a lin_z on every block, no view mean
    2: (1, 0, 6, 1),       # smallest: no lin_z, no projection
    3: (1, 1, 6, 1),       # one block with lin_z
    4: (8, 8, 6, 1),       # largest: 24 packed layers, 25 scale slots, all 8 lin_z entries
    5: (8, 0, 6, 3),       # view mean directly after lin_in, every block per point
    6: (8, 7, 6, 3),       # view mean before the last block
    7: (2, 1, 6, 2),       # smallest multi-view case with both loop kinds
    8: (5, 3, 0, 1),       # pe_n = 0, d_in = 6: empty PE buffers
    9: (5, 3, 1, 1),       # pe_n = 2, d_in = 12
    10: (5, 3, 8, 1),      # pe_n = 16, d_in = 54: full PE table, fourth lin_in k-block
    11: (5, 5, 6, 1),      # the boundary of combine_layer < n_blocks
}
ALL = sorted(DESCS)


def did(i):
    return "d%d_%d_%d_%d_%d" % ((i,) + DESCS[i])


def mlp_conf(nb, cl):
    return dict(type="resnet", n_blocks=nb, d_hidden=512, combine_layer=cl, combine_type="average")


def model_conf(coarse, fine=None, num_freqs=6):
    """tgp.model_conf with num_freqs and a separate fine MLP shape: coarse / fine = (n_blocks,
    combine_layer)."""
    c = tgp.model_conf()
    c["code"] = dict(c["code"], num_freqs=num_freqs)
    c["mlp_coarse"] = mlp_conf(*coarse)
    c["mlp_fine"] = mlp_conf(*(fine or coarse))
    return c


def state(seed, coarse, fine=None, num_freqs=6):
    """synth.pixelnerf_state; with ``fine`` a fine MLP of another shape (its own seed, as there)."""
    d_in = 6 + 6 * num_freqs
    sd = synth.pixelnerf_state(seed, d_in=d_in, n_blocks=coarse[0], combine_layer=coarse[1], num_freqs=num_freqs)
    if fine is not None and fine != coarse:
        for k in [k for k in sd if k.startswith("mlp_fine.")]:
            del sd[k]
        sd.update(synth.resnetfc_state(seed + 1, d_in, 512, 512, fine[0], fine[1], prefix="mlp_fine."))
    return sd


def make_net(conf, sd, precision="f16x3", latent_proj=True):
    net = PixelNeRFNet(conf)
    net.mlp_precision = precision
    net.use_latent_proj = latent_proj
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("encoder.") for k in missing), (missing, unexpected)
    return net.to(DEV).eval()


def oracle_fn(sd, scene, coarse, fine=None):
    """model_fn of ref_cpu.render / a point query for a (possibly mixed-shape) model."""
    fine = fine or coarse

    def fn(pts, is_coarse, dirs):
        nb, cl = coarse if is_coarse else fine
        return ref_cpu.pixelnerf_forward(sd, scene, pts, is_coarse, dirs, n_blocks=nb, combine_layer=cl)

    return fn


# ---- the point-query scene (test_point_query_multiview_multiobject_vs_oracle's) ----------------
P_QUERY = 200      # per object: three full 64-point tiles and a tile of 8


def query_scene(ns):
    sb = 2 if ns > 1 else 1
    lat = synth.latent(9, sb * ns, 512, 12, 16)
    poses = synth.srn_poses([-20.0 + 15 * i for i in range(sb * ns)], radius=1.6).reshape(sb, ns, 4, 4)
    focal = torch.tensor([[60.0, 64.0], [70.0, 66.0]])[:sb]
    c = torch.tensor([[31.0, 30.0], [33.0, 29.0]])[:sb]
    xyz = torch.from_numpy(synth.hash_sym(77, (sb, P_QUERY, 3), 0.5))
    vd = torch.nn.functional.normalize(torch.from_numpy(synth.hash_sym(78, (sb, P_QUERY, 3), 1.0)), dim=-1)
    return dict(sb=sb, lat=lat, poses=poses, focal=focal, c=c, xyz=xyz, vd=vd,
                scene=ref_cpu.Scene(lat, poses, focal, 64, 60, c))


def encode_query(net, q):
    net.encode_latent(q["lat"].to(DEV), q["poses"].to(DEV), q["focal"].to(DEV), (64, 60), c=q["c"].to(DEV),
                      num_objs=q["sb"])


@functools.lru_cache(maxsize=None)
def query_refs(i, emulate=False):
    """(scene record, state dict, oracle output[, emulation output]) of descriptor i, computed once."""
    nb, cl, nf, ns = DESCS[i]
    q = query_scene(ns)
    sd = state(4, (nb, cl), num_freqs=nf)
    fn = oracle_fn(sd, q["scene"], (nb, cl))
    with torch.no_grad():
        ref = fn(q["xyz"], True, q["vd"])
    assert torch.isfinite(ref).all() and float(ref[..., 3].max()) > 0    # sigma not all clipped
    emu = with_emulation(lambda: fn(q["xyz"], True, q["vd"])) if emulate else None
    return q, sd, ref, emu


# ---- C6 (host part): refused before any launch ------------------------------------------------
def _pack_rc(desc):
    """pnr_mlp_pack's status and message for ``desc`` with valid pointers everywhere."""
    lib = _lib.load()
    t = torch.zeros(512 * 512, device=DEV)
    w = _lib.MlpWeights()
    w.desc = desc
    for name in ("lin_in_w", "lin_in_b", "lin_out_w", "lin_out_b", "pe_freqs", "pe_phases"):
        setattr(w, name, t.data_ptr())
    for arr in (w.lin_z_w, w.lin_z_b, w.fc0_w, w.fc0_b, w.fc1_w, w.fc1_b):
        for j in range(8):
            arr[j] = t.data_ptr()
    out = torch.full((4096,), 7.0, device=DEV)
    rc = lib.pnr_mlp_pack(w, _lib.ptr(out), 1 << 40, _lib.stream_of(torch.device(DEV)))
    msg = lib.pnr_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused pack wrote to its output"
    return rc, msg


@pytest.mark.parametrize("what,desc,rcs,word", [
    ("pe_n = 17", (6 + 3 * 17, 512, 512, 4, 5, 3, 17, 0), (-2,), b"pe_n"),
    ("n_blocks = 0", (42, 512, 512, 4, 0, 3, 12, 0), (-2,), b"n_blocks"),
    ("n_blocks = 9", (42, 512, 512, 4, 9, 3, 12, 0), (-2,), b"n_blocks"),
    ("combine_layer = -1", (42, 512, 512, 4, 5, -1, 12, 0), (-1,), b"combine_layer"),
    ("d_in != 6 + 3 pe_n", (41, 512, 512, 4, 5, 3, 12, 0), (-2,), b"d_in"),
], ids=["pe_n17", "nb0", "nb9", "cl-1", "d_in"])
def test_pack_refuses_descriptors_outside_the_range(what, desc, rcs, word):
    """pnr_mlp_pack returns PNR_ERR_UNSUPPORTED (-2) / PNR_ERR_INVALID (-1) with its message, and
    pnr_mlp_packed_bytes 0, before any launch (the output buffer is untouched)."""
    d = _lib.MlpDesc(*desc)
    assert _lib.load().pnr_mlp_packed_bytes(d) == 0, what
    rc, msg = _pack_rc(d)
    assert rc in rcs and word in msg, (what, rc, msg)


def test_pack_accepts_the_range_ends():
    lib = _lib.load()
    for nb, cl, pe_n in ((1, 0, 0), (8, 8, 16), (8, 1000, 16)):
        assert lib.pnr_mlp_packed_bytes(_lib.MlpDesc(6 + 3 * pe_n, 512, 512, 4, nb, cl, pe_n, 3)) > 0


def test_point_query_refuses_views_without_a_view_mean():
    """pnr_point_query with NS = 2 and combine_layer >= n_blocks (no view mean in the model):
    PNR_ERR_UNSUPPORTED before any launch; the model reports the same reason."""
    lib = _lib.load()
    lat = torch.zeros(2, 4, 4, 512, device=DEV)
    cams = torch.zeros(2, 16, device=DEV)
    sc = _lib.Scene(lat.data_ptr(), cams.data_ptr(), 1, 2, 4, 4, 512, 32.0, 32.0)
    xyz = torch.zeros(8, 3, device=DEV)
    out = torch.full((8, 4), 7.0, device=DEV)
    ws = torch.zeros(1 << 20, device=DEV)
    for nb, cl in ((3, 1000), (5, 5)):
        d = _lib.MlpDesc(42, 512, 512, 4, nb, cl, 12, 0)
        rc = lib.pnr_point_query(sc, d, _lib.ptr(ws), _lib.ptr(xyz), None, 8, _lib.ptr(out), _lib.ptr(ws),
                                 ws.numel() * 4, _lib.stream_of(torch.device(DEV)))
        assert rc == -2 and b"combine_layer < n_blocks" in lib.pnr_last_error(), (rc, lib.pnr_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    q = query_scene(2)
    net = make_net(model_conf((3, 1000)), state(4, (3, 1000)))
    encode_query(net, q)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="combine_layer < n_blocks"):
        net(q["xyz"].to(DEV), coarse=True, viewdirs=q["vd"].to(DEV))


# ---- C1: point query against the oracle ---------------------------------------------------------
def _point_query(i, precision, latent_proj):
    nb, cl, nf, ns = DESCS[i]
    q, sd, ref, _ = query_refs(i)
    net = make_net(model_conf((nb, cl), num_freqs=nf), sd, precision, latent_proj)
    assert net.fused_conf_reason() is None and net.d_in == 6 + 6 * nf
    encode_query(net, q)
    if cl == 0:
        assert net.hip_proj(True) is None      # no lin_z layers: nothing to project
    with torch.no_grad():
        out = net(q["xyz"].to(DEV), coarse=True, viewdirs=q["vd"].to(DEV))
    torch.cuda.synchronize()
    d = (out.cpu() - ref).abs()
    print("%s %s proj=%s: max |d| %.3e, worst |d| / tolerance %.3f (max |ref| %.2f)" % (
        did(i), precision, latent_proj, float(d.max()), float((d / (tgp.ATOL + tgp.RTOL * ref.abs())).max()),
        float(ref.abs().max())))
    tgp.assert_close(out, ref, "point query %s %s" % (did(i), precision))


@pytest.mark.parametrize("latent_proj", [True, False])
@pytest.mark.parametrize("i", ALL, ids=did)
def test_point_query_fp32_vs_oracle(i, latent_proj):
    _point_query(i, "fp32", latent_proj)


@pytest.mark.parametrize("latent_proj", [True, False])
@pytest.mark.parametrize("precision", [p for p in tgp.PRECS if p != "fp32"])
@pytest.mark.parametrize("i", ALL, ids=did)
def test_point_query_split_precisions_vs_oracle(i, precision, latent_proj):
    _point_query(i, precision, latent_proj)


# ---- C2: the "f16" mode, bounded by the emulation ----------------------------------------------
@pytest.mark.parametrize("i", [1, 4, 6, 10], ids=did)
def test_point_query_f16_bounded_by_emulation(i):
    nb, cl, nf, ns = DESCS[i]
    q, sd, ref, emu = query_refs(i, True)
    net = make_net(model_conf((nb, cl), num_freqs=nf), sd, "f16")
    encode_query(net, q)
    with torch.no_grad():
        out = net(q["xyz"].to(DEV), coarse=True, viewdirs=q["vd"].to(DEV))
    bounded_raw(out, ref, emu, did(i))


# ---- C3: render -----------------------------------------------------------------------------------
N_RAYS, KC, KF = 96, 64, 64
# the streams' seeds were chosen on the CPU among 1 .. 20 (1 .. 12 for descriptor 6 and the mixed
# models): the fp32 oracle against an fp64 oracle (state dict, latent, rays and streams as
# doubles) flips no ray's fine bins, and the draws keep the largest distance to a cdf boundary
# (smallest / second smallest over the 96 rays: 9.8e-6 / 1.2e-5, 1.0e-6 / 4.8e-6, 5.2e-6 / 6.3e-6)
RENDER = {1: dict(kfd=0, stream_seed=14), 6: dict(kfd=16, stream_seed=4), 10: dict(kfd=0, stream_seed=20)}
MIXED_STREAM_SEED = 2    # 1.6e-6 / 3.2e-6 and 1.7e-6 / 7.4e-6 for the two mixed models


def render_scene(i):
    nb, cl, nf, ns = DESCS[i]
    if ns == 1:
        sc = synth.scene_srn(seed=5, n_rays=N_RAYS, pick="hash")
        return dict(sb=1, lat=sc["latent"], poses=sc["poses"], focal=sc["focal"], wh=(128, 128),
                    rays=sc["rays"][None].contiguous())
    sb = 2
    lat = synth.latent(10, sb * ns, 512, 30, 40)
    poses = synth.srn_poses([30.0 * k for k in range(sb * ns)], radius=1.4).reshape(sb, ns, 4, 4)
    focal = torch.tensor(90.0)
    rays = util.gen_rays(synth.srn_poses([15.0 + 40.0 * k for k in range(sb)], radius=1.4), 96, 80, focal,
                         0.4, 2.4).reshape(sb, -1, 8)
    idx = torch.from_numpy((synth.hash_uniform(3, N_RAYS // sb) * rays.shape[1]).astype("int64"))
    return dict(sb=sb, lat=lat, poses=poses, focal=focal, wh=(96, 80), rays=rays[:, idx].contiguous())


def ref_arrays(ref, rays, streams):
    """ref_cpu.render's output as the array dict tgp.compare_render reads."""
    return dict(coarse_rgb=ref["coarse"]["rgb"], coarse_depth=ref["coarse"]["depth"],
                coarse_weights=ref["coarse"]["weights"], fine_rgb=ref["fine"]["rgb"],
                fine_depth=ref["fine"]["depth"], fine_weights=ref["fine"]["weights"], z_fine=ref["fine"]["z"],
                z_coarse=ref["coarse"]["z"], rays=rays, u_coarse=streams[0], u_fine=streams[1],
                u_fine_jit=streams[2], n_depth=streams[3])


@functools.lru_cache(maxsize=None)
def render_refs(i):
    nb, cl, nf, ns = DESCS[i]
    s = render_scene(i)
    sd = state(1, (nb, cl), num_freqs=nf)
    kfd = RENDER[i]["kfd"]
    streams = synth.rng_streams(RENDER[i]["stream_seed"], N_RAYS, KC, KF, kfd)
    scene = ref_cpu.Scene(s["lat"], s["poses"], s["focal"], s["wh"][0], s["wh"][1], None)
    with torch.no_grad():
        ref = ref_cpu.render(oracle_fn(sd, scene, (nb, cl)), s["rays"], KC, KF, kfd, streams, True)
    return s, sd, scene, streams, ref


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("i", sorted(RENDER), ids=did)
def test_render_march_modes_and_oracle(i, precision):
    """96 rays, 64 + 64 samples (16 depth samples for the multi-view descriptor, so that march
    mode 3 applies to the other two).  (a) March modes 1, 2, 3 are bit-identical to mode 0 in
    rgb, depth, weights and z, as in test_fused_march_matches_unfused.  (b) Mode 0 against
    ref_cpu.render at the project tolerance, with the proven-flip rule of
    test_render_multiobject_vs_oracle (tgp.compare_render, MAX_FLIPS = 1); the streams' seeds
    (RENDER) leave no flip to the oracle's own rounding."""
    nb, cl, nf, ns = DESCS[i]
    s, sd, scene, streams, ref = render_refs(i)
    kfd = RENDER[i]["kfd"]
    net = make_net(model_conf((nb, cl), num_freqs=nf), sd, precision)
    net.encode_latent(s["lat"].to(DEV), s["poses"].to(DEV), s["focal"].to(DEV), s["wh"], num_objs=s["sb"])
    r = NeRFRenderer(n_coarse=KC, n_fine=KF, n_fine_depth=kfd, white_bkgd=True)
    r.return_z = True
    rays = s["rays"].to(DEV)
    outs = []
    for mode in (0, 1, 2, 3):
        r.march_mode = mode
        r.streams = streams
        with torch.no_grad():
            outs.append(r(net, rays, want_weights=True))
    torch.cuda.synchronize()
    b = outs[0]
    for mode in (1, 2, 3):
        for p in ("coarse", "fine"):
            for k in ("rgb", "depth", "weights", "z"):
                x, y = outs[mode][p][k], b[p][k]
                assert torch.equal(x, y), (mode, p, k, float((x - y).abs().max()))
    n = tgp.compare_render("%s/%s" % (did(i), precision), b, dict(n_fine=KF, n_fine_depth=kfd),
                           ref_arrays(ref, s["rays"], streams),
                           oracle=(sd, scene, dict(n_blocks=nb, combine_layer=cl), True, N_RAYS // s["sb"]))
    print("%s/%s: proven fine-bin flips %d" % (did(i), precision, n))


# ---- C6: routes ---------------------------------------------------------------------------------
def test_num_freqs_10_point_query_takes_the_callback_path():
    """NeRF's usual num_freqs = 10 (pe_n = 20, d_in = 66) is outside pnr_mlp_pack's range: the
    model takes the callback path and matches the oracle (it used to raise from packed())."""
    q = query_scene(1)
    sd = state(4, (5, 3), num_freqs=10)
    with torch.no_grad():
        ref = oracle_fn(sd, q["scene"], (5, 3))(q["xyz"], True, q["vd"])
    net = make_net(model_conf((5, 3), num_freqs=10), sd)
    assert "positional encoding" in net.fused_conf_reason() and net.d_in == 66
    encode_query(net, q)
    with torch.no_grad():
        out = net(q["xyz"].to(DEV), coarse=True, viewdirs=q["vd"].to(DEV))
    tgp.assert_close(out, ref, "num_freqs = 10 point query")


MIXED = [((5, 3), (3, 1000)), ((3, 1000), (5, 3))]


@pytest.mark.parametrize("coarse,fine", MIXED, ids=["c5_3_f3_1000", "c3_1000_f5_3"])
def test_mixed_shape_model_takes_the_callback_path(coarse, fine, monkeypatch):
    """mlp_fine of another shape than mlp_coarse: pnr_render_forward* take one descriptor for both
    packs, so the model must never reach them (with the smaller fine pack the fine pass would
    read past its end).  Point queries of both MLPs and a 96-ray 64 + 48 + 16 render match the
    oracle through the callback path; no fused render call is made."""
    sd = state(4, coarse, fine)
    net = make_net(model_conf(coarse, fine), sd)
    assert "different shape" in net.fused_conf_reason()
    called = []

    def refuse_fused_call(self, *a, **k):
        called.append(1)
        raise AssertionError("a mixed-shape model reached the single-descriptor fused render call")

    monkeypatch.setattr(NeRFRenderer, "_fused_call", refuse_fused_call)
    q = query_scene(1)
    encode_query(net, q)
    for is_coarse in (True, False):
        with torch.no_grad():
            ref = oracle_fn(sd, q["scene"], coarse, fine)(q["xyz"], is_coarse, q["vd"])
            out = net(q["xyz"].to(DEV), coarse=is_coarse, viewdirs=q["vd"].to(DEV))
        tgp.assert_close(out, ref, "mixed point query coarse=%s" % is_coarse)
    kfd = 16
    sc = synth.scene_srn(seed=5, n_rays=N_RAYS, pick="hash")
    rays = sc["rays"][None].contiguous()
    streams = synth.rng_streams(MIXED_STREAM_SEED, N_RAYS, KC, KF, kfd)
    scene = ref_cpu.Scene(sc["latent"], sc["poses"], sc["focal"], 128, 128, None)
    with torch.no_grad():
        ref = ref_cpu.render(oracle_fn(sd, scene, coarse, fine), rays, KC, KF, kfd, streams, True)
    net.encode_latent(sc["latent"].to(DEV), sc["poses"].to(DEV), sc["focal"].to(DEV), (128, 128))
    r = NeRFRenderer(n_coarse=KC, n_fine=KF, n_fine_depth=kfd, white_bkgd=True)
    r.streams = streams
    r.return_z = True
    with torch.no_grad():
        out = r(net, rays.to(DEV), want_weights=True)
    torch.cuda.synchronize()
    assert not called
    out = DotMap(coarse=DotMap(out["coarse"]), fine=DotMap(out["fine"]))
    tgp.compare_render("mixed %s/%s" % (coarse, fine), out, dict(n_fine=KF, n_fine_depth=kfd),
                       ref_arrays(ref, rays, streams),
                       oracle=(sd, scene, dict(n_blocks=fine[0], combine_layer=fine[1]), True, N_RAYS))
