"""Drop-in for the reference's ``simple_knn`` package (submodules/simple-knn): ``simple_knn._C.distCUDA2`` on the HIP
kernel ``gs2m_knn_mean_dist2``.  ``scene/gaussian_model.py:20`` imports ``distCUDA2`` from ``simple_knn._C`` at module scope;

    import sys, gs2mesh_amd.simple_knn
    sys.modules["simple_knn"] = gs2mesh_amd.simple_knn
    sys.modules["simple_knn._C"] = gs2mesh_amd.simple_knn._C

makes that import resolve here."""
from . import _C  # noqa: F401
from ._C import distCUDA2  # noqa: F401
