"""Expert sharding and the last hidden widths 96, 160, 192 and 224: they run the fused output-layer kernels on one GPU (and data-parallel), but not as expert
shards - ep.can_shard keeps refusing them, and keeps accepting 32, 64, 128 and 256.  No GPU needed."""
import pytest

from opentf_amd.ep import can_shard


@pytest.mark.parametrize("W", (96, 160, 192, 224))
def test_can_shard_refuses_the_widths_served_by_a_wider_template(W):
    assert not can_shard([128, W, 233_629], 2)
    assert not can_shard([128, 64, W, 233_629], 8)
    assert not can_shard([W, 233_629], 2)             # a no-hidden-layer model whose input has that width


@pytest.mark.parametrize("W", (32, 64, 128, 256))
def test_can_shard_still_accepts_the_template_widths(W):
    assert can_shard([128, W, 233_629], 2)
    assert can_shard([128, W, 233_629], 8)
