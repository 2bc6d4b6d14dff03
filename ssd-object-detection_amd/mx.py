"""Host-side storage of block-scaled fp8 (MX e4m3) operands: the (q, scale) pair of a map, and a flat bf16 range quantised in
one launch whose per-tensor pairs are slices of the result."""
import math

from . import ops


def pair(shape, device):
    """Uninitialised (q u8 [..., C], scale u8 [..., C/32]) of the MX-fp8 form of a [..., C] map."""
    assert shape[-1] % 32 == 0, shape
    return ops._mx_pair(shape, device)


class FlatStore:
    """The MX-fp8 form of ONE flat bf16 range (a stretch of the engine's filters), from ONE ops.quantize_mx_fp8 over it; the
    pair of a tensor inside the range is a slice of the result (view).  Nothing exists until the first quantize().

    The range is quantised again at EVERY fp8 forward / backward and nothing is cached against the weights: no path that
    writes the bf16 filters (optimizer step, load_state_dict, refresh_weights) can leave a stale fp8 copy behind."""

    def __init__(self):
        self.q = self.scale = None
        self._views = {}                       # (offset, shape) -> the pair view() built: the walks ask per layer, per step

    @property
    def allocated(self):
        """Whether any fp8 run has happened (a bf16-only run allocates nothing)."""
        return self.q is not None

    def adopt(self, q, scale):
        """Use these flat uint8 buffers (q [n], scale [n / 32]) as the store."""
        assert q.dim() == scale.dim() == 1 and q.numel() == scale.numel() * 32, (tuple(q.shape), tuple(scale.shape))
        self.q, self.scale, self._views = q, scale, {}
        return self

    def quantize(self, src_flat):
        """(Re)quantise the whole range from src_flat (bf16 [n], n % 32 == 0): one launch."""
        if self.q is None:
            self.adopt(*pair((src_flat.numel(),), src_flat.device))
        ops.quantize_mx_fp8(src_flat, q=self.q, scale=self.scale)

    def view(self, offset, shape):
        """(q [shape], scale [shape[:-1] + (C/32,)]) of the tensor of `shape` that starts `offset` elements into the range.
        Both must be whole 32-element blocks: a tensor's scale bytes are then the slice at offset / 32."""
        shape = tuple(shape)
        v = self._views.get((offset, shape))
        if v is None:
            n = math.prod(shape)
            assert offset >= 0 and offset % 32 == 0 and shape[-1] % 32 == 0, (offset, shape)
            assert offset + n <= self.q.numel(), (offset, n, self.q.numel())
            v = self._views[offset, shape] = (self.q[offset:offset + n].view(shape),
                                              self.scale[offset // 32:(offset + n) // 32].view(shape[:-1] + (shape[-1] // 32,)))
        return v
