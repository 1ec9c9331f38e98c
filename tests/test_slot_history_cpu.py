"""Keeps the poison list of tests/test_slot_history.py complete (no GPU, the native library is not loaded).

Every device buffer the engine passes to its kernels is a pointer-typed field of the ctypes mirror of ndp_engine.  The slot-history
tests overwrite those buffers with garbage before a pair is loaded; a buffer that is missing from their list is a buffer whose stale
contents no test looks at.  So a field added to the struct fails here until someone decides: poisoned, or exempt for a reason."""
import ctypes

from tests._helpers import ENGINE_POISON_EXEMPT, ENGINE_POISONED


def _pointer_fields():
    from deformationpyramid_amd import _native as N
    loaded = N._LIB                                        # (another test of the session may have loaded it; this one must not)
    fields = [name for name, ctype in N.Engine._fields_ if ctype is ctypes.c_void_p or issubclass(ctype, ctypes._Pointer)]
    assert N._LIB is loaded, "reading the struct's fields must not load the shared library"
    return fields


def test_every_engine_buffer_is_poisoned_or_exempt_for_a_reason():
    fields = _pointer_fields()
    assert len(fields) >= 20, fields                       # the mirror still declares its buffers as pointers
    undecided = [f for f in fields if f not in ENGINE_POISONED and f not in ENGINE_POISON_EXEMPT]
    assert not undecided, f"engine buffers that the slot-history tests neither poison nor exempt: {undecided}"


def test_the_two_lists_name_only_buffers_that_exist_and_do_not_overlap():
    fields = set(_pointer_fields())
    assert len(set(ENGINE_POISONED)) == len(ENGINE_POISONED)
    assert not set(ENGINE_POISONED) - fields, set(ENGINE_POISONED) - fields
    assert not set(ENGINE_POISON_EXEMPT) - fields, set(ENGINE_POISON_EXEMPT) - fields
    assert not set(ENGINE_POISONED) & set(ENGINE_POISON_EXEMPT)
    for name, reason in ENGINE_POISON_EXEMPT.items():
        assert isinstance(reason, str) and len(reason.split()) >= 4, name        # a reason, not a placeholder


def test_the_decision_constants_are_those_of_the_header():
    """The slot-history tests tell how a level ended from PairState.decision: _native's DEC_* must be the header's NDP_DEC_* enum."""
    import os
    import re

    from deformationpyramid_amd import _native as N
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "ndp_hip.h")) as f:
        enum = dict((k, int(v)) for k, v in re.findall(r"NDP_(DEC_[A-Z_]+)\s*=\s*(\d+)", f.read()))
    assert enum == dict(DEC_STEP=N.DEC_STEP, DEC_ADVANCE=N.DEC_ADVANCE, DEC_STEP_ADVANCE=N.DEC_STEP_ADVANCE, DEC_IDLE=N.DEC_IDLE), enum


def test_the_engine_hands_every_buffer_of_the_lists_to_the_struct():
    """The names are attributes BatchedEngine._mk_struct copies into the struct: a renamed tensor would otherwise leave the
    poisoning a silent no-op (the GPU test skips attributes an engine does not have -- the nnc_* buffers exist only with nn_cells)."""
    import inspect

    from deformationpyramid_amd.engine import BatchedEngine
    src = inspect.getsource(BatchedEngine._mk_struct)
    for name in list(ENGINE_POISONED) + list(ENGINE_POISON_EXEMPT):
        assert f'"{name}"' in src, name
