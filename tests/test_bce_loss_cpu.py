"""CPU-side checks of the classification additions: `conan_bce_loss_fwd` is exported and refuses bad arguments before any launch (no pointer is
dereferenced on the host, and there is no device here), and the new names resolve where the existing model classes do."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from conan_fgw_amd import _lib
    return _lib


def test_bce_loss_entry_point_is_exported_and_in_the_ctypes_table(built):
    assert hasattr(ctypes.CDLL(built.library_path()), "conan_bce_loss_fwd")
    res, args = built.SIGNATURES["conan_bce_loss_fwd"]
    assert res is ctypes.c_int and len(args) == 8
    assert built.ABI_VERSION == 6                                         # an added export: the version stays


def test_bce_loss_rejects_bad_arguments_without_launching(built):
    L = built.lib()
    buf = (ctypes.c_float * 8)()                                          # host memory standing in for the pointers: never dereferenced before the checks
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.conan_bce_loss_fwd(None, None, None, 0, 5, None, None, None) == -1      # all null
    for hole in range(4):                                                            # each of pred / target / loss / dpred on its own
        a = [p, p, p, p]
        a[hole] = None
        assert L.conan_bce_loss_fwd(a[0], a[1], None, 0, 5, a[2], a[3], None) == -1, hole
    assert L.conan_bce_loss_fwd(p, p, None, 0, 0, p, p, None) == -1                  # n = 0
    assert L.conan_bce_loss_fwd(p, p, None, 0, -3, p, p, None) == -1
    assert L.conan_bce_loss_fwd(p, p, p, 2, 5, p, p, None) == -1                     # n_weight outside {0, 1, n}
    assert L.conan_bce_loss_fwd(p, p, p, -1, 5, p, p, None) == -1
    assert L.conan_bce_loss_fwd(p, p, None, 1, 5, p, p, None) == -1                  # a weight announced, none given
    assert L.conan_bce_loss_fwd(p, p, None, 5, 5, p, p, None) == -1


def test_new_model_classes_and_loss_are_exported_like_their_siblings():
    import conan_fgw_amd
    from conan_fgw_amd import head
    for name in ("EmbeddingsWithGATAggregationClassification", "EmbeddingsWithGAT", "classification_loss", "EmbeddingsWithGATAggregation",
                 "EmbeddingsWithGATAggregationBaryCenter", "EmbeddingsWithGATAggregationClassificationBaryCenter"):
        assert getattr(conan_fgw_amd, name) is getattr(head, name)
    assert issubclass(head.EmbeddingsWithGATAggregationClassification, head.EmbeddingsWithGATAggregationClassificationBaryCenter)


def test_forward_dummy_returns_none_on_cpu_tensors_without_a_model_on_the_gpu():
    """`load_dummy` (model/utils.py:23-33) calls forward_dummy on a CPU mini-batch before the model moves to the GPU; it touches no sub-module."""
    import torch
    from conan_fgw_amd.head import EmbeddingsWithGAT, EmbeddingsWithGATAggregationClassification
    for cls in (EmbeddingsWithGATAggregationClassification, EmbeddingsWithGAT):
        m = cls.__new__(cls)                                              # no constructor: the backbones allocate on the device
        assert cls.forward_dummy(m, torch.zeros(3), torch.zeros(3, dtype=torch.long), torch.zeros(3, dtype=torch.long)) is None
