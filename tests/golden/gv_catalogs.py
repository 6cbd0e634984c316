"""The reference's GV diagram catalogs that the tests read (data files of its src/frontend/GV_diagrams: the sigma catalogs of
orders 1-4 with GOrder, VerOrder <= 2, Vertex4<n> for n = 1-4, Vertex4I3/I4, and Polar<n> for n = 1-5 in groups_charge and
groups_spin), stored as one compressed archive, GV_diagrams.tar.xz, and unpacked once per process into a temporary directory."""
import atexit
import os
import shutil
import tarfile
import tempfile

ARCHIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "GV_diagrams.tar.xz")
_root = None


def root():
    """A directory laid out like the reference's src/frontend/GV_diagrams (groups_sigma/, groups_vertex4/, groups_charge/, groups_spin/)."""
    global _root
    if _root is None:
        d = tempfile.mkdtemp(prefix="gv_catalogs_")
        atexit.register(shutil.rmtree, d, True)
        with tarfile.open(ARCHIVE) as tf:
            tf.extractall(d, filter="data")
        _root = os.path.join(d, "GV_diagrams")
    return _root
