"""``eioku_amd._handle.Handle`` driven by a stand-in library: a plain object whose ``eioku_fake_*`` attributes are Python
callables that record their calls.  No GPU and no shared library are involved."""
import ctypes as C
import gc

import numpy as np
import pytest

from eioku_amd._handle import Handle
from eioku_amd._lib import EiokuHipError

CONVS = [("stem", 4, 3, 3, 2), ("layer1.0", 8, 4, 1, 1)]
TENSORS = [("embed.weight", 5, 3), ("embed.bias", 1, 3)]
POINTER = 0x1000  # what the stand-in's create hands out; never dereferenced


class Fake:
    """``eioku_fake_*``.  ``stride=False`` gives ``conv_info`` the CRAFT / CRNN signature, without the stride output."""

    def __init__(self, stride: bool = True):
        self.calls, self.set, self.conv_outs = [], {}, 4 if stride else 3
        # ctypes functions carry their argtypes; these two are the ones the handle reads them from
        self.eioku_fake_conv_info = self._with_argtypes(self._conv_info, 4 + self.conv_outs)
        self.eioku_fake_tensor_info = self._with_argtypes(self._tensor_info, 6)

    @staticmethod
    def _with_argtypes(method, n):
        def fn(*args):
            return method(*args)

        fn.argtypes = [None] * n
        return fn

    def _handle(self, h, what):
        self.calls.append(what)
        assert isinstance(h, C.c_void_p) and h.value == POINTER, "the library was handed something that is not the handle"

    def eioku_last_error(self):
        return b"fake error"

    def eioku_fake_create(self, a, b, out):
        self.calls.append(("create", a, b))
        out._obj.value = POINTER
        return 0

    def eioku_fake_other_create(self, out):
        self.calls.append("other_create")
        out._obj.value = POINTER
        return 0

    def eioku_fake_destroy(self, h):
        self._handle(h, "destroy")

    def eioku_fake_num_convs(self, h):
        self._handle(h, "num_convs")
        return len(CONVS)

    def _conv_info(self, h, i, name, cap, *outs):
        self._handle(h, "conv_info")
        assert cap == len(name) and len(outs) == self.conv_outs
        name.value = CONVS[i][0].encode()
        for o, v in zip(outs, CONVS[i][1:]):
            o._obj.value = v
        return 0

    def eioku_fake_set_conv(self, h, i, w, b):
        self._handle(h, "set_conv")
        _, cout, cin, k, _ = CONVS[i]
        self.set[CONVS[i][0]] = (np.ctypeslib.as_array((C.c_float * (cout * cin * k * k)).from_address(w)).copy(),
                                 np.ctypeslib.as_array((C.c_float * cout).from_address(b)).copy())
        return 0

    def eioku_fake_num_tensors(self, h):
        self._handle(h, "num_tensors")
        return len(TENSORS)

    def _tensor_info(self, h, i, name, cap, rows, cols):
        self._handle(h, "tensor_info")
        name.value = TENSORS[i][0].encode()
        rows._obj.value, cols._obj.value = TENSORS[i][1:]
        return 0

    def eioku_fake_set_tensor(self, h, i, data, n):
        self._handle(h, "set_tensor")
        self.set[TENSORS[i][0]] = np.ctypeslib.as_array((C.c_float * n).from_address(data)).copy()
        return 0

    def eioku_fake_last_ms(self, h, a, b):
        self._handle(h, "last_ms")
        a._obj.value, b._obj.value = 1.5, 2.5
        return 0

    def eioku_fake_forward(self, h, x):
        self._handle(h, "forward")
        return -3 if x < 0 else 0


def handle(fake=None):
    fake = fake or Fake()
    return Handle("fake", 7, 9, lib=fake), fake


def conv_state(rng):
    return {n: (rng.standard_normal((co, ci, k, k)), rng.standard_normal(co)) for n, co, ci, k, _ in CONVS}


def test_create_passes_the_arguments_and_the_create_name_can_be_given():
    h, fake = handle()
    assert fake.calls == [("create", 7, 9)] and h and h.ptr.value == POINTER
    other = Handle("fake", create="eioku_fake_other_create", lib=fake)
    assert fake.calls[-1] == "other_create"
    other.close()
    assert fake.calls[-1] == "destroy"


def test_convs_and_tensors_are_what_the_library_reports():
    h, _ = handle()
    assert h.convs() == CONVS
    assert h.tensors() == TENSORS
    h, _ = handle(Fake(stride=False))
    assert h.convs() == [(*c[:4], None) for c in CONVS]


def test_set_convs_hands_over_contiguous_fp32_of_the_right_contents():
    h, fake = handle()
    state = conv_state(np.random.default_rng(0))
    w = np.asfortranarray(state["stem"][0])                       # float64 and not C-contiguous
    state["stem"] = (w, state["stem"][1])
    state["layer1.0"] = (state["layer1.0"][0][:, :, 0, 0], state["layer1.0"][1])   # a 1 x 1 convolution given as a matrix
    h.set_convs(state)
    for name, (w, b) in state.items():
        assert np.array_equal(fake.set[name][0], w.astype(np.float32).ravel()), name
        assert np.array_equal(fake.set[name][1], b.astype(np.float32)), name


def test_set_convs_takes_a_per_layer_callable():
    h, fake = handle()
    seen = []

    def layer(name, cout, cin, k):
        seen.append((name, cout, cin, k))
        return np.full((cout, cin, k, k), len(seen)), np.zeros(cout)

    h.set_convs(layer)
    assert seen == [c[:4] for c in CONVS]
    assert (fake.set["stem"][0] == 1).all() and (fake.set["layer1.0"][0] == 2).all()


def test_set_tensors_takes_a_mapping_or_a_callable():
    h, fake = handle()
    h.set_tensors({"embed.weight": np.arange(15.0).reshape(5, 3).T.copy().T, "embed.bias": [1, 2, 3]})
    assert np.array_equal(fake.set["embed.weight"], np.arange(15, dtype=np.float32))
    assert np.array_equal(fake.set["embed.bias"], np.array([1, 2, 3], np.float32))
    seen = []

    def make(name, rows, cols):
        seen.append((name, rows, cols))
        return np.full(rows * cols, 4.0)

    h.set_tensors(make)
    assert seen == TENSORS and (fake.set["embed.weight"] == 4).all()


def test_doubles_returns_every_output():
    h, _ = handle()
    assert h.doubles("last_ms", 2) == (1.5, 2.5)


def bad_states():
    rng = np.random.default_rng(1)
    missing = conv_state(rng)
    del missing["layer1.0"]
    weight = conv_state(rng)
    weight["stem"] = (np.zeros((4, 3, 3, 2)), weight["stem"][1])
    bias = conv_state(rng)
    bias["stem"] = (bias["stem"][0], np.zeros(5))
    return [("set_convs", missing, KeyError, "layer1.0"), ("set_convs", weight, ValueError, "stem"),
            ("set_convs", bias, ValueError, "stem"),
            ("set_tensors", {"embed.weight": np.zeros(15)}, KeyError, "embed.bias"),
            ("set_tensors", {"embed.weight": np.zeros(14), "embed.bias": np.zeros(3)}, ValueError, "embed.weight")]


@pytest.mark.parametrize("method, state, error, layer", bad_states(),
                         ids=["missing conv", "weight shape", "bias shape", "missing tensor", "tensor size"])
def test_a_failed_load_names_the_layer_and_closes_the_handle_once(method, state, error, layer):
    """The constructor rule: ``handle.or_close(load, ...)`` destroys the handle before the exception leaves."""
    h, fake = handle()
    with pytest.raises(error, match=layer.replace(".", r"\.")):
        h.or_close(getattr(h, method), state)
    assert fake.calls.count("destroy") == 1 and not h
    h.close()
    del h
    gc.collect()
    assert fake.calls.count("destroy") == 1


def test_a_failing_library_call_raises_with_the_librarys_message():
    h, _ = handle()
    with pytest.raises(EiokuHipError, match=r"eioku_fake_forward failed \(code -3\): fake error"):
        h.check(h.eioku_fake_forward(-1), "eioku_fake_forward")


def test_close_twice_destroys_once():
    h, fake = handle()
    assert h.eioku_fake_forward(1) == 0
    h.close()
    h.close()
    assert fake.calls.count("destroy") == 1 and not h


def test_a_closed_handle_is_refused_before_the_library_sees_a_call():
    h, fake = handle()
    h.eioku_fake_forward(1)                                        # bound and cached while the handle lives
    h.close()
    seen = list(fake.calls)
    for use in (lambda: h.eioku_fake_forward(1), h.convs, h.tensors, lambda: h.set_convs({}), lambda: h.set_tensors({}),
                lambda: h.doubles("last_ms", 2), lambda: h.ptr, lambda: h._as_parameter_):
        with pytest.raises(EiokuHipError, match="fake handle is closed"):
            use()
    assert fake.calls == seen


def test_a_live_handle_is_a_ctypes_argument_and_a_closed_one_is_not():
    fn = C.CFUNCTYPE(C.c_void_p, C.c_void_p)(lambda p: p)             # the identity, with argtypes as the library's functions have
    h, _ = handle()
    assert fn(h) == POINTER
    h.close()
    with pytest.raises(C.ArgumentError, match="fake handle is closed"):
        fn(h)


def test_collection_destroys_an_unclosed_handle_once():
    h, fake = handle()
    del h
    gc.collect()
    assert fake.calls.count("destroy") == 1
