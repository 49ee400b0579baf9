"""The deferred anchor head of PointPillarKITTI (backbone_head -> class map + DeferredHead record; box / direction logits computed at
the selected anchors by csrc/head_rows.hip): consistent with its own all-anchor materialisation, equal to the full 72-column head
within the head tolerance, an error once its concat buffers were overwritten, and no change for plain head tensors.  Whole-batch and
two-stream split forward (LIDAR_BEV_SPLIT_MIN lowered through the module's list cell so that a batch of 2 splits)."""
import pytest
import torch

from lidardetection_amd import _lib, bev_backbone as bb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model_canvas(dev):
    from lidardetection_amd.pointpillar import PointPillarKITTI
    m = PointPillarKITTI(batch_size=2, device=dev).randomize_for_bench(3)
    g = torch.Generator(device="cpu").manual_seed(11)
    canvas = torch.randn(2, 64, m.ny, m.nx, generator=g).to(dev)
    canvas[:, :, ::3] = 0
    return m, canvas.contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("split", [False, True])
def test_deferred_head_post_process_and_full_head(model_canvas, monkeypatch, split):
    m, canvas = model_canvas
    monkeypatch.setattr(bb, "_SPLIT_MIN", [1 if split else 8])
    monkeypatch.setattr(bb, "_HEAD_DEFER", [True])
    bev = m._bev_folded()
    with torch.no_grad():
        bev._streams = None
        (head,) = m.backbone_head(canvas)
        assert (bev._streams is not None) == split
        rec = head.deferred
        assert head.shape == (2, m.ny // 2, m.nx // 2, 18) and len(rec.parts) == (2 if split else 1) and not rec.stale()
        # consistency: the selected anchors' logits are the all-anchor materialisation's, so both routes give the same detections
        fused = m.post_process(head)
        cls, box, dirs = m.split_heads(head)
        plain = m.post_process(cls, box, dirs)
        for x, y, name in zip(fused, plain, ("boxes", "scores", "labels", "counts")):
            assert torch.equal(x, y), name
        assert int(fused[3].min()) > 0 and bool(torch.isfinite(fused[0]).all())
        cls, box, dirs = cls.clone(), box.clone(), dirs.clone()
        # against the full head of the same input
        (full,) = m.backbone_head(canvas, defer=False)
        assert full.shape[-1] == 72 and getattr(full, "deferred", None) is None
        for a, b, name in zip((cls, box, dirs), m.split_heads(full), ("cls", "box", "dir")):
            assert a.shape == b.shape, name
            err = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
            print(f"[head defer split={split}] {name} err/scale vs the full head {err:.1e}")
            assert err <= 1e-4, (name, err)
        # the full-head forward overwrote the concat buffers: the first head is stale now
        assert rec.stale()


def test_stale_deferred_head_raises(model_canvas, monkeypatch):
    m, canvas = model_canvas
    monkeypatch.setattr(bb, "_HEAD_DEFER", [True])
    with torch.no_grad():
        (first,) = m.backbone_head(canvas)
        (second,) = m.backbone_head(canvas)
        with pytest.raises(_lib.LidarHipError, match="stale"):
            m.post_process(first)
        with pytest.raises(_lib.LidarHipError, match="stale"):
            m.split_heads(first)
        out = m.post_process(second)                      # repeated backbone_head calls, the last one post-processed: valid
        assert int(out[3].min()) > 0


def test_switch_off_and_plain_head_tensor(model_canvas, monkeypatch):
    m, canvas = model_canvas
    monkeypatch.setattr(bb, "_HEAD_DEFER", [False])
    with torch.no_grad():
        (head,) = m.backbone_head(canvas)
        assert head.shape[-1] == 72 and getattr(head, "deferred", None) is None
        # a plain (B, H, W, 72) tensor built by the caller: today's path, equal to the torch ops on its three heads
        g = torch.Generator(device="cpu").manual_seed(17)
        plain_head = torch.randn(2, m.ny // 2, m.nx // 2, 72, generator=g)
        plain_head[..., :18] *= 3.0
        plain_head[..., 18:60] *= 0.3
        plain_head = plain_head.to(canvas.device)
        for h in (head, plain_head):
            for x, y in zip(m.post_process(h), m.post_process(*m.split_heads(h))):
                assert torch.equal(x, y)
