"""The memory contract of an entry of include/facegen_hip.h, checked on the device: it writes nothing but its outputs and its
workspace, leaves its inputs alone, reads nothing it did not write itself (outputs, workspace, the bytes behind an input) and needs
no more workspace than the size function states.  Helper module, imported like gpu_util.

Arena: ONE device allocation per test.  Every operand is a view inside it with a guard band of at least max(1 MiB, its own size) on
both sides, so an overrun of a kernel under test lands inside the allocation.  Guards hold a fixed non-NaN 32-bit pattern (the bands
behind the inputs are re-filled per run, see run_contract) and are compared as int32 against a host-planned expectation.  A view is
exactly as long as asked -- the guard starts at the next float -- and starts at EXACTLY the requested alignment (address % (2 *
align) == align): 256 bytes unless the header promises less ("16-byte aligned"), never less than it states."""
import numpy as np
import torch

PATTERN = 0x5A5AA5A5                 # as fp32: 1.5387e16, finite; as int32: positive
MIB_FLOATS = (1 << 20) // 4
NAN_BITS = 0x7FC00000
FILLS = (float("nan"), 0.0, 1e30)    # what outputs and workspaces hold before run 1, 2, 3
TAIL_FILLS = (NAN_BITS, 0, PATTERN)  # what the guard band behind every input holds in run 1, 2, 3 (int32 bits)


class Arena:
    def __init__(self, device, mib=64):
        self.n = mib * MIB_FLOATS
        self.buf = torch.empty(self.n, dtype=torch.float32, device=device)     # the one allocation the kernels see
        self.bits = self.buf.view(torch.int32)
        self.bits.fill_(PATTERN)
        self.expect = torch.full_like(self.bits, PATTERN)                       # guards: expected bits; views: ignored
        self.is_guard = torch.ones(self.n, dtype=torch.bool, device=device)
        self.views = []              # (start, n, name) in floats, ascending
        self._end, self._end_guard = 0, 0     # end of the last view; the guard it asked for behind itself

    @classmethod
    def sized(cls, device, sizes):
        """an arena that holds views of these float counts with their guard bands"""
        # (a view pays the larger of its own guard and its predecessor's in front of it)
        need = sum(n + 2 * max(MIB_FLOATS, n) + 128 for n in sizes) + max([MIB_FLOATS] + list(sizes)) + MIB_FLOATS
        return cls(device, -(-need // MIB_FLOATS))

    def take(self, n_floats, align=256, name=None):
        """-> a float32 view of exactly n_floats (>= 1)."""
        n = int(n_floats)
        assert n >= 1
        guard = max(MIB_FLOATS, n)
        a = align // 4
        assert align % 4 == 0 and a & (a - 1) == 0
        lo = self._end + max(guard, self._end_guard)
        base = self.buf.data_ptr() // 4
        start = lo + (a - (base + lo) % (2 * a)) % (2 * a)      # address % (2 * align) == align: aligned to `align`, and no more
        assert (base + start) % (2 * a) == a
        if start + n + guard > self.n:
            raise AssertionError("arena of %d MiB too small for %s (%d floats)" % (self.n // MIB_FLOATS, name, n))
        self.is_guard[start:start + n] = False
        self.views.append((start, n, name or "view%d" % len(self.views)))
        self._end, self._end_guard = start + n, guard
        return self.buf[start:start + n]

    def put(self, array, align=256, name=None):
        """take() + copy of a numpy array / tensor (any dtype of 4 bytes); returns the view shaped like the array."""
        t = torch.as_tensor(np.ascontiguousarray(array) if isinstance(array, np.ndarray) else array)
        v = self.take(t.numel(), align, name)
        if t.dtype == torch.int32:
            v.view(torch.int32).copy_(t.reshape(-1))
        else:
            v.copy_(t.reshape(-1).to(torch.float32))
        return v.view(t.shape)

    def _span(self, v):
        at = (v.data_ptr() - self.buf.data_ptr()) // 4
        for i, (s, n, name) in enumerate(self.views):
            if s == at:
                nxt = self.views[i + 1][0] if i + 1 < len(self.views) else self.n
                return s, n, name, nxt
        raise KeyError("not a view of this arena")

    def fill_tail(self, v, bits):
        """The whole guard band behind view v (up to the next view) <- bits; assert_guards expects them there."""
        s, n, _, nxt = self._span(v)
        self.bits[s + n:nxt] = bits
        self.expect[s + n:nxt] = bits

    def assert_guards(self, what=""):
        bad = (self.bits != self.expect) & self.is_guard
        if not bool(bad.any()):
            return
        idx = torch.nonzero(bad).reshape(-1)
        first, last = int(idx[0]), int(idx[-1])
        msgs = []
        for off in (first, last):
            # the nearest view: the one whose end lies before off, or whose start lies after it
            best = min(self.views, key=lambda sv: min(abs(off - sv[0]), abs(off - (sv[0] + sv[1]))))
            s, n, name = best
            msgs.append("%s[%d] (%s, a view of %d floats)" % (name, off - s, "%d floats before its start" % (s - off) if off < s else
                                                               "%d floats past its last element" % (off - (s + n) + 1), n))
        raise AssertionError("%s: %d guard floats disturbed; first at %s, last at %s; first value bits 0x%08x"
                             % (what, idx.numel(), msgs[0], msgs[1], int(self.bits[first]) & 0xFFFFFFFF))


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def run_contract(arena, call, inputs, outputs, workspaces=(), inout=(), what="", fills=FILLS):
    """Runs `call()` once per fill.  inputs / outputs / workspaces: views of the arena; inout: (view, initial tensor) pairs that the
    entry updates in place (restored before every run, compared like outputs).  Before run i the outputs and workspaces hold
    fills[i] and the guard band behind every input and every workspace holds TAIL_FILLS[i] (a read past the end of either meets NaN).  Asserts: (1) every guard untouched, (2) the inputs
    bit-identical after the call, (3) the results of all runs bit-identical -- with NaN in the first fill: nothing is read before it is
    written, every pad is written and not assumed --, (4) no NaN in any result.  Returns the results (clones, outputs then in-outs) of
    the last run for the caller's comparison with the oracle."""
    snap = [_bits(v).clone() for v in inputs]
    first = None
    for i, fill in enumerate(fills):
        for v in list(outputs) + list(workspaces):
            v.fill_(fill)
        for v, init in inout:
            v.copy_(init.reshape(v.shape))
        for v in list(inputs) + list(workspaces):
            arena.fill_tail(v, TAIL_FILLS[i])
        call()
        torch.cuda.synchronize()
        tag = "%s [prefill %r]" % (what, fill)
        arena.assert_guards(tag)
        for k, (v, s) in enumerate(zip(inputs, snap)):
            assert torch.equal(_bits(v), s), "%s: input %d was written" % (tag, k)
        res = [v.clone() for v in outputs] + [v.clone() for v, _ in inout]
        for k, r in enumerate(res):
            if r.dtype == torch.float32:
                assert not bool(torch.isnan(r).any()), "%s: NaN in result %d (%d of %d)" % (tag, k, int(torch.isnan(r).sum()), r.numel())
        if first is None:
            first = res
        else:
            for k, (a, b) in enumerate(zip(first, res)):
                if not torch.equal(_bits(a), _bits(b)):
                    d = torch.nonzero(_bits(a).reshape(-1) != _bits(b).reshape(-1)).reshape(-1)
                    raise AssertionError("%s: result %d depends on what the outputs / workspace / input tails held before: %d of %d "
                                         "elements differ from the NaN-prefilled run, first at %d (%r vs %r)"
                                         % (tag, k, d.numel(), a.numel(), int(d[0]), float(a.reshape(-1)[d[0]]), float(b.reshape(-1)[d[0]])))
    for v in list(inputs) + list(workspaces):
        arena.fill_tail(v, PATTERN)
    return res


def run_accumulate(arena, call_beta1, acc_outputs, beta0_results, inputs, workspaces=(), what=""):
    """The fourth run of a beta / acc entry: the accumulating outputs hold a known finite prefill, call_beta1() runs with beta = 1
    (workspaces poisoned with NaN).  Returns [(got, prefill + beta0_result)] as float64 numpy pairs for the caller's bar."""
    gen = torch.Generator().manual_seed(1234)
    pre = [torch.randn(v.numel(), generator=gen).reshape(v.shape).to(v.device) for v in acc_outputs]
    for v, p in zip(acc_outputs, pre):
        v.copy_(p)
    for v in workspaces:
        v.fill_(float("nan"))
    snap = [_bits(v).clone() for v in inputs]
    call_beta1()
    torch.cuda.synchronize()
    arena.assert_guards(what + " [beta = 1]")
    for k, (v, s) in enumerate(zip(inputs, snap)):
        assert torch.equal(_bits(v), s), "%s [beta = 1]: input %d was written" % (what, k)
    return [(v.cpu().numpy().astype(np.float64), p.cpu().numpy().astype(np.float64) + r.cpu().numpy().astype(np.float64))
            for v, p, r in zip(acc_outputs, pre, beta0_results)]
