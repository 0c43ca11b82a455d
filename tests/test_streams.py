"""The stage table of tests/test_streams_gpu.py (tests/_streams.py) is complete: every public reader of a recording and every
public stage on a trace matrix has a case that runs it off the default stream, and every constructor that initialises device state
asynchronously is in the regime that feeds it on another stream.  A stage added later cannot arrive without a stream test.

Needs neither torch nor the library: the pipeline modules import without them."""
import importlib
import inspect
import os
import pkgutil
import re

import _streams as st

import deep_calcium_amd
from deep_calcium_amd._matrix import _MatrixStage
from deep_calcium_amd._reader import _FrameReader

HERE = os.path.dirname(os.path.abspath(__file__))


def _public_stages():
    """{name: class} of the public classes of every module of the package that names one of the two bases or the extractor that
    leads a second reader: the subclasses of _FrameReader and _MatrixStage, and the owners of a _LeadingExtractor."""
    found = {}
    for info in pkgutil.iter_modules(deep_calcium_amd.__path__):
        path = os.path.join(deep_calcium_amd.__path__[0], info.name + '.py')
        if not os.path.isfile(path):
            continue
        with open(path) as fp:
            if not re.search(r'_FrameReader|_MatrixStage|_LeadingExtractor|RoiTraceExtractor', fp.read()):
                continue
        module = importlib.import_module('deep_calcium_amd.' + info.name)
        for name, cls in vars(module).items():
            if name.startswith('_') or not inspect.isclass(cls) or cls.__module__ != module.__name__:
                continue
            if issubclass(cls, (_FrameReader, _MatrixStage)) or '_LeadingExtractor(' in inspect.getsource(cls):
                found[name] = cls
    return found


def test_the_walk_finds_the_stages_it_is_meant_to_find():
    names = set(_public_stages())
    assert {'SeriesSummarizer', 'TemporalBinner', 'FrameQuality', 'FrameFilter', 'MotionCorrector', 'BidiEstimator', 'RoiTraceExtractor',
            'WeightedTraceExtractor', 'RoiFootprints', 'RoiPairCorr', 'TraceBaseline', 'TracePairCorr', 'TraceDynamics',
            'TraceDeconvolver'} <= names


def test_every_public_stage_has_a_stream_case():
    stages = _public_stages()
    readers = set(c.cls for c in st.READERS)
    matrix = set(c.cls for c in st.MATRIX)
    for name, cls in stages.items():
        assert name in (matrix if issubclass(cls, _MatrixStage) else readers), '%s has no case in tests/_streams.py' % name
    assert readers | matrix <= set(stages), 'a case names a class that is not a public stage: %r' % sorted((readers | matrix) - set(stages))


def test_every_asynchronous_constructor_is_fed_on_another_stream():
    """A reader whose constructor (its own, or the one it inherits) fills with torch.zeros / torch.full or launches a kernel has
    a case with init= set, and its constructor ends with _constructed(), which feed() waits for."""
    stages = _public_stages()
    delayed = set(c.cls for c in st.READERS if c.init is not None)
    for name, cls in stages.items():
        if issubclass(cls, _MatrixStage):
            continue
        src = inspect.getsource(cls.__init__)
        if re.search(r'torch\.(zeros|full)\(|self\.L\.dc_\w+\(', src):
            assert name in delayed, '%s initialises device state asynchronously: give a case init=' % name
        assert '_constructed()' in src, '%s.__init__ does not end with _constructed()' % name


def test_the_gpu_file_runs_the_whole_table():
    with open(os.path.join(HERE, 'test_streams_gpu.py')) as fp:
        src = fp.read()
    for use in ('st.params(st.READERS,', 'st.params(st.MATRIX,', 'only=lambda c: c.init is not None'):
        assert use in src, use
    ids = [c.id for c in st.READERS + st.MATRIX]
    assert len(ids) == len(set(ids))
