from ..alignments import Alignments
from .alignment import alignment
from .cosine import cosine
from .euclidean import euclidean
from .fit_alignment import fit_alignment
from .hamming import hamming
from .levenshtein import levenshtein, levenshtein_knn
from .local_alignment import local_alignment
from .minkowski import minkowski
from .profile_alignment import profile_alignment
from .semiglobal_alignment import semiglobal_alignment
from .spectrum import spectrum
from .substitution import substitution
from .utils import clean_input
