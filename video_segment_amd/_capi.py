"""What the ctypes layers of libvsg_render, libvsg_flow and libvsg_resize (render.py, flow.py,
resize.py) share: loading a library, turning a status into a VsgError, option structs from keyword
arguments, pointers to the caller's frames, and the life of a handle."""
import ctypes as C
import os
import subprocess

from ._lib import VSG_MEM_DEVICE, VSG_MEM_HOST, VSG_OK, VsgError

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path(name):
    return os.path.join(_HERE, "lib", "lib%s.so" % name)


def make(subdir, force=False):
    """Compiles the library of video_segment_amd/<subdir> in-tree; make decides what is stale."""
    subprocess.check_call(["make", "-C", os.path.join(_HERE, subdir), "-j8", "-s"] + (["-B"] if force else []))


def load(path, what):
    if not os.path.exists(path):
        raise RuntimeError("%s is missing (%s): build the HIP extension first; there is no "
                           "fallback path" % (what, path))
    try:   # one HIP runtime per process: bind to the one torch loaded (see _lib.lib)
        import torch  # noqa: F401
    except ImportError:
        pass
    return C.CDLL(path)


def checker(prefix, last_error):
    """check(rc) of a library: raises VsgError("<prefix> error <rc>: <last error>") for a failure."""
    def check(rc):
        if rc != VSG_OK:
            raise VsgError("%s error %d: %s" % (prefix, rc, last_error().decode()), rc)
    return check


def default_options(struct, default_fn, what, **kw):
    o = struct()
    default_fn(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError("unknown %s option %r" % (what, k))
        setattr(o, k, v)
    return o


class Structure(C.Structure):
    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def is_torch(x):
    return type(x).__module__.startswith("torch")


def _memory(x):
    """(address, strides in bytes or elements, mem kind) of a numpy array or torch tensor."""
    if not is_torch(x):
        return x.ctypes.data, x.strides, VSG_MEM_HOST
    return x.data_ptr(), tuple(x.stride()), VSG_MEM_DEVICE if x.is_cuda else VSG_MEM_HOST


def _drain(x):
    """The libraries work on streams of their own: torch's stream of a CUDA tensor is drained first."""
    if is_torch(x) and x.is_cuda:
        import torch
        torch.cuda.current_stream(x.device).synchronize()


def frame_ptr(x, rows, width, channels, what, expected=None, unpacked="pixels have to be packed"):
    """(pointer, row stride in bytes, mem kind) of a rows x width x channels uint8 array or tensor
    (rows x width for one channel) whose pixels are packed and whose rows may be further apart.
    expected: how the ValueError names the shape; unpacked: how it names pixels that are not packed."""
    shape = (rows, width, channels) if channels > 1 else (rows, width)
    if tuple(x.shape) != shape:
        raise ValueError("%s has to be %s, got %s" % (what, expected or " x ".join(map(str, shape)), tuple(x.shape)))
    if str(x.dtype).replace("torch.", "") != "uint8":
        raise TypeError("%s has to be uint8" % what)
    ptr, strides, mem = _memory(x)
    # the stride of an axis of length 1 says nothing (numpy leaves a slice's there): it is not looked at
    packed = (width == 1 or strides[1] == channels) and (channels == 1 or strides[2] == 1)
    if not packed or (rows > 1 and strides[0] < channels * width):
        raise ValueError("%s: %s" % (what, unpacked))
    _drain(x)
    return C.c_void_p(ptr), strides[0] if rows > 1 else channels * width, mem


def contiguous_ptr(out):
    """(pointer, mem kind) of a contiguous numpy array or torch tensor the library is to fill."""
    if is_torch(out):
        if not out.is_contiguous():
            raise ValueError("out has to be contiguous")
    elif not out.flags["C_CONTIGUOUS"]:
        raise ValueError("out has to be C-contiguous")
    ptr, _, mem = _memory(out)
    _drain(out)
    return C.c_void_p(ptr), mem


class Handle:
    """A vsg_X handle in self.h and the library's destroy function in self._destroy, both set by the
    subclass; destroyed by close() or with the object."""

    def close(self):
        if getattr(self, "h", None):
            self._destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()
