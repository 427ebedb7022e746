"""The row-view helpers and the call check that the fused ops of ``freegaussian_amd.ops`` share, on CPU tensors and their
metadata alone: ``_rows`` hands a tensor on as it is where its rows are ``width`` consecutive floats a fixed number (>= width)
of floats apart and copies it otherwise, ``_row_stride`` is the stride the entry points are given (the width where there is at
most one row), and ``_gpu_float32`` refuses a CPU tensor with an ``FgRasterError`` that names the op."""
import pytest
import torch

from freegaussian_amd import _lib, ops


def _as_is(t, width, stride):
    r = ops._rows(t, width)
    assert r is t
    assert ops._row_stride(r, width) == stride


def _copied(t, width):
    r = ops._rows(t, width)
    assert r is not t and r.is_contiguous() and r.data_ptr() != t.data_ptr()
    assert torch.equal(r, t)
    assert ops._row_stride(r, width) == width


def test_rows_passes_contiguous_rows_and_columns_of_a_block_as_they_are():
    _as_is(torch.randn(5, 3), 3, 3)
    heads13 = torch.randn(5, 13)
    _as_is(heads13[:, 0:3], 3, 13)
    _as_is(heads13[:, 3:6], 3, 13)
    _as_is(torch.randn(5, 10)[:, 3:7], 4, 10)


def test_row_stride_of_at_most_one_row_is_the_width():
    one = torch.randn(5, 13)[2:3, 3:6]  # (torch keeps 13 as the stride of the one row)
    _as_is(one, 3, 3)
    _as_is(torch.randn(5, 10)[4:5, 3:7], 4, 4)
    _as_is(torch.empty(0, 3), 3, 3)
    _as_is(torch.empty(0, 4), 4, 4)
    _as_is(torch.empty(0, 13)[:, 3:6], 3, 3)


def test_rows_copies_what_is_not_rows_of_consecutive_floats():
    _copied(torch.randn(3, 5).T, 3)  # [5,3] with the floats of a row 5 apart
    _copied(torch.randn(5, 6)[:, ::2], 3)  # a column step of 2
    _copied(torch.randn(5, 8)[:, ::2], 4)
    _copied(torch.randn(8).as_strided((5, 3), (1, 1)), 3)  # rows 1 float apart: they overlap


class _OnGpu:
    """What ``_gpu_float32`` reads of a tensor, with ``is_cuda`` set."""

    def __init__(self, t):
        self.is_cuda, self.dtype, self.device = True, t.dtype, t.device


def test_shared_call_check_refuses_cpu_tensors_by_op_name():
    a = torch.randn(5, 3)
    with pytest.raises(_lib.FgRasterError, match=r"some_op runs on the GPU only \(b is a CPU tensor; the torch statement\)"):
        ops._gpu_float32("some_op", "the torch statement", None, b=a)
    with pytest.raises(_lib.FgRasterError, match="GPU only") as e:
        ops._gpu_float32("some_op", "the torch statement", torch.device("cpu"), a=a.double(), b=a)
    assert "some_op" in str(e.value)  # (the CPU tensor comes before any dtype)
    # the second pass, reached without a GPU through stand-ins that say they are on one
    with pytest.raises(ValueError, match="some_op: float32 tensors on cpu expected, got b: torch.float64 on cpu"):
        ops._gpu_float32("some_op", "the torch statement", a.device, a=_OnGpu(a), b=_OnGpu(a.double()))
    with pytest.raises(ValueError, match="got b: torch.float32 on meta"):
        ops._gpu_float32("some_op", "the torch statement", a.device, a=_OnGpu(a), b=_OnGpu(a.to("meta")))
    ops._gpu_float32("some_op", "the torch statement", a.device, a=_OnGpu(a), b=_OnGpu(a.clone()))
    ops._gpu_float32("some_op", "the torch statement", None, a=_OnGpu(a), b=_OnGpu(a.double()))  # (None: the op converts)
    for call, name in (
        (lambda: ops.se3_apply(a, a.clone(), a.clone()), "se3_apply"),
        (lambda: ops.color_correct(a, a.clone()), "color_correct"),
        (lambda: ops.bilagrid_apply(torch.randn(2, 12, 4, 5, 6), 0, torch.randn(7, 9, 3)), "bilagrid_apply"),
    ):
        with pytest.raises(_lib.FgRasterError, match="GPU only") as e:
            call()
        assert name in str(e.value)
