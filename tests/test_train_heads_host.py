"""What the training step reports about its attention at the reference's smaller widths (no GPU needed): `-cs 256` / `-cs 128` with the
model's 8 heads are head dims 32 / 16, which the split-fp16 attention kernels of train_attn.hip take like head dim 64; head dim 8
(`-cs 64`) and the cross-check switch D3DP_TRAIN_ATTN=f32 stay on the fp32 attention."""
from types import SimpleNamespace

import pytest

from d3dp_amd import D3DP
from d3dp_amd.weights import H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT

X2_BOTH = "attention of both axes, forward and backward, on split-fp16 operands"


def arithmetic(cs, frames=27):
    args = SimpleNamespace(number_of_frames=frames, test_time_augmentation=True, timestep=1000, scale=1.0, cs=cs, dep=2)
    return D3DP(args, H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, is_train=True).pose_estimator.train_arithmetic()


@pytest.mark.parametrize("cs", [512, 256, 128])
def test_matrix_core_head_dims_report_split_fp16_attention_of_both_axes(monkeypatch, cs):
    monkeypatch.delenv("D3DP_TRAIN_ATTN", raising=False)
    monkeypatch.delenv("D3DP_TRAIN_IMPL", raising=False)
    text = arithmetic(cs)
    assert X2_BOTH in text and "fp32 attention" not in text, text


@pytest.mark.parametrize("cs", [256, 128])
def test_cross_check_switch_reports_the_fp32_attention(monkeypatch, cs):
    monkeypatch.delenv("D3DP_TRAIN_IMPL", raising=False)
    monkeypatch.setenv("D3DP_TRAIN_ATTN", "f32")
    text = arithmetic(cs)
    assert "fp32 attention" in text and X2_BOTH not in text, text


def test_head_dim_8_still_reports_the_fp32_attention(monkeypatch):
    monkeypatch.delenv("D3DP_TRAIN_ATTN", raising=False)
    monkeypatch.delenv("D3DP_TRAIN_IMPL", raising=False)
    text = arithmetic(64)
    assert "fp32 attention" in text and X2_BOTH not in text, text
