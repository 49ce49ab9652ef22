from .exact import GP, ExactGP
from .basic import BasicGP
from .gradobs import GradientGP
from .multiout import MultiOutputGP
from .coreg import CoregionalGP
from .laplace import LaplaceGP
from .sparse_laplace import SparseLaplaceGP
from .ep import EPGP
from .sparse_ep import SparseEPGP
from .softmax import MulticlassLaplaceGP
from .fitc import FITC
from .dtc import DTC
from .vfe import VFE
from .select import select_pseudoinputs
from .fourier import FourierSample
from .ssgp import SSGP
from .pathwise import PathwiseSample
from .iterative import IterativeGP

__all__ = ['GP', 'ExactGP', 'BasicGP', 'GradientGP', 'MultiOutputGP', 'CoregionalGP', 'LaplaceGP',
           'SparseLaplaceGP', 'EPGP', 'SparseEPGP', 'MulticlassLaplaceGP', 'FITC', 'DTC', 'VFE', 'select_pseudoinputs', 'FourierSample', 'SSGP',
           'PathwiseSample', 'IterativeGP']
