"""GP models (gptorch/models/__init__.py:20-21)."""
from .base import GPModel  # noqa: F401
from .gpr import GPR  # noqa: F401
from ._lockstep import batched_factorise, batched_log_likelihood, batched_loss_and_grad, release_batch_buffers  # noqa: F401
from ._multistart import multi_start_optimize  # noqa: F401
from .sparse_gpr import SVGP, VFE  # noqa: F401
from ._fitc import FITC  # noqa: F401
from .dist_gpr import DistGPR  # noqa: F401
from .laplace import LaplaceGP  # noqa: F401
from .ep import EPGP  # noqa: F401
