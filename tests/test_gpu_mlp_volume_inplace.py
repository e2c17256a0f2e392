"""The metadata-MLP sweep reads the matching encoder's channels-last buffer in place (sr_mlp_volume_fwd_nhwc) instead of
copying both operands to [B,16,h,w] / [B,K,16,h,w] and packing the source features back (sr_mlp_volume_fwd).  The values a
lane loads are the same, so the two entry points must agree bit for bit; and a view the in-place path cannot read -- a
channel slice of a wider buffer, a base address off the 16-byte grid, true NCHW -- must take the copy path and give the
same bits again.  Which entry point ran is counted at the library binding, not inferred from the results."""
import pytest
import torch

from simplerecon_amd import _lib, synthetic
from simplerecon_amd import cost_volume as cv

DEV = "cuda:0"
B, C = 2, 16
MAPS = [(24, 32), (20, 24)]   # whole 8x8 tiles; ragged tiles on both edges
ENTRIES = ("sr_mlp_volume_fwd", "sr_mlp_volume_fwd_nhwc")


def _encoder_like_feats(K, h, w, seed):
    """cur [B,16,h,w] and src [B,K,16,h,w] as ResnetMatchingEncoder.forward_pair returns them: two slices of ONE
    channels-last [B(1+K),16,h,w] buffer."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    buf = torch.randn((B * (1 + K), h, w, C), generator=g).to(DEV).permute(0, 3, 1, 2)
    return buf[:B], buf[B:].unflatten(0, (B, K))


@pytest.fixture
def entry_calls(monkeypatch):
    """{entry point: calls} of the two forward entry points, counted through the object _lib.lib() hands out."""
    real, counts = _lib.lib(), dict.fromkeys(ENTRIES, 0)

    class Counting:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name not in counts:
                return fn

            def counted(*args):
                counts[name] += 1
                return fn(*args)
            return counted

    monkeypatch.setattr(_lib, "lib", lambda: Counting())
    return counts


def _run(mgr, poses, cur, src):
    with torch.inference_mode():
        vol, lowest, _, mask = mgr(return_mask=True, **dict(poses, cur_feats=cur, src_feats=src))
    torch.cuda.synchronize()
    return vol, lowest, mask


def _setup(K, D, h, w):
    mgr = cv.FeatureVolumeManager(h, w, num_depth_bins=D, matching_dim_size=C, num_source_views=K)
    synthetic.seeded_fill_(mgr.mlp, seed=50 + K)
    poses = {k: v.to(DEV) for k, v in synthetic.cost_volume_inputs(B, K, C, h, w, seed=7 + K).items()
             if k not in ("cur_feats", "src_feats")}
    return mgr.to(DEV), poses


def _assert_same(got, want, what):
    for name, g, t in zip(("volume", "lowest_cost", "mask"), got, want):
        assert torch.equal(g, t), f"{what}: {name} differs"


def test_dense_channels_last_pair_predicate():
    """Host logic (no GPU): exactly the dense channels-last slice pairs qualify."""
    K, h, w = 3, 5, 6
    buf = torch.zeros(B * (1 + K), h, w, C).permute(0, 3, 1, 2)
    cur, src = buf[:B], buf[B:].unflatten(0, (B, K))
    ok = cv.dense_channels_last_pair
    assert ok(cur, src)
    assert ok(cur[:1], src[:1])                                       # a batch of one: its stride addresses nothing
    assert not ok(cur.contiguous(), src.contiguous())                 # true NCHW
    assert not ok(cur, src.contiguous()) and not ok(cur.contiguous(), src)
    assert not ok(cur.double(), src.double())
    wide = torch.zeros(B * (1 + K), h, w, 2 * C).permute(0, 3, 1, 2)[:, :C]
    assert not ok(wide[:B], wide[B:].unflatten(0, (B, K)))            # channel slice: pixel stride 32
    assert not ok(cur[:, :, :, :w - 1], src[:, :, :, :, :w - 1])      # a column slice: row stride is the wider map's
    assert not ok(cur, src[:, :K - 1])                                # a view slice: frame stride spans K views
    flat = torch.zeros(buf.numel() + 1)
    off = flat[1:].view(B * (1 + K), h, w, C).permute(0, 3, 1, 2)
    assert off.data_ptr() % 16 == 4
    assert not ok(off[:B], off[B:].unflatten(0, (B, K)))              # 4 bytes off the 16-byte grid
    assert not ok(cur[0], src[0])                                     # wrong rank


@pytest.mark.gpu
@pytest.mark.parametrize("hw", MAPS, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("D", [8, 12])
@pytest.mark.parametrize("K", [2, 7, 9])   # K = 9: W2 no longer fits the LDS beside W1, the second instantiation
def test_in_place_equals_copy_path(entry_calls, K, D, hw):
    h, w = hw
    mgr, poses = _setup(K, D, h, w)
    cur, src = _encoder_like_feats(K, h, w, seed=11 * K + D + h)
    assert cv.dense_channels_last_pair(cur, src) and not cur.is_contiguous()

    in_place = _run(mgr, poses, cur, src)
    assert entry_calls == {"sr_mlp_volume_fwd": 0, "sr_mlp_volume_fwd_nhwc": 1}
    copied = _run(mgr, poses, cur.contiguous(), src.contiguous())
    assert entry_calls == {"sr_mlp_volume_fwd": 1, "sr_mlp_volume_fwd_nhwc": 1}
    assert torch.isfinite(copied[0]).all() and copied[0].std() > 0
    _assert_same(in_place, copied, f"K={K} D={D} {h}x{w}")

    # the channels-last volume (16-byte stores of a unit's planes) reads in place too
    mgr.volume_memory_format = torch.channels_last
    vol_cl = _run(mgr, poses, cur, src)[0]
    assert entry_calls["sr_mlp_volume_fwd_nhwc"] == 2 and torch.equal(vol_cl.contiguous(), copied[0])


@pytest.mark.gpu
def test_views_that_cannot_be_read_in_place_take_the_copy_path(entry_calls):
    K, D, (h, w) = 2, 8, MAPS[1]
    mgr, poses = _setup(K, D, h, w)
    cur, src = _encoder_like_feats(K, h, w, seed=5)
    want = _run(mgr, poses, cur, src)
    assert entry_calls == {"sr_mlp_volume_fwd": 0, "sr_mlp_volume_fwd_nhwc": 1}

    both = torch.cat([cur, src.flatten(0, 1)])                         # [B(1+K),16,h,w], the values of the buffer
    wide = torch.full((B * (1 + K), h, w, 2 * C), 7.0, device=DEV).permute(0, 3, 1, 2)
    wide[:, :C] = both
    flat = torch.full((both.numel() + 1,), 7.0, device=DEV)
    off = flat[1:].view(B * (1 + K), h, w, C).permute(0, 3, 1, 2)
    off.copy_(both)
    assert off.data_ptr() % 16 == 4
    views = {"channel slice of a 32-channel buffer": wide[:, :C], "base address 4 bytes off": off,
             "true NCHW": both.contiguous()}
    for n, (what, t) in enumerate(views.items(), 1):
        assert torch.equal(t, both)
        got = _run(mgr, poses, t[:B], t[B:].unflatten(0, (B, K)))
        assert entry_calls == {"sr_mlp_volume_fwd": n, "sr_mlp_volume_fwd_nhwc": 1}, what
        _assert_same(got, want, what)
