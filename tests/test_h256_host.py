"""Expert sharding at a last hidden width of 256 (the exact-f32 fused output-layer kernels): which models ep.can_shard accepts.  No GPU needed."""
from opentf_amd.ep import can_shard


def test_can_shard_accepts_a_last_hidden_width_of_256():
    assert can_shard([128, 256, 233_629], 8)
    assert can_shard([128, 64, 256, 3000], 2)


def test_can_shard_still_refuses_other_widths_and_too_few_tiles():
    assert not can_shard([128, 192, 233_629], 2)      # no fused kernels at this width: the generic chain, data parallelism
    assert not can_shard([18, 256, 112], 2)           # one 256-expert tile for two ranks
