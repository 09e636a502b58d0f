"""Guarded scratch for the workspace contract of the C ABI (include/s2anet_hip.h, "Workspaces").

GuardedWorkspaces(fill) stands in for s2anet_amd._lib.workspace(nbytes, device, tag): every request gets a FRESH buffer of
exactly the declared number of bytes, pre-filled with one byte value and surrounded by canaries of the same value:

    [ FRONT canary | nbytes handed out | nbytes + BACK canary ]

An entry point that overruns its declaration by less than nbytes + 64 KiB writes into the canary -- check() finds it --
and not outside the allocation.  The production helper cannot show any of this: it hands out at least 64 KiB, grows and
never shrinks, and keeps the previous call's contents.

    gw = GuardedWorkspaces(0xA5)
    monkeypatch.setattr(_lib, "workspace", gw)     # every Python wrapper calls _lib.workspace through the module attribute
    ...
    gw.check()
"""
import torch

FRONT = 4096
BACK = 65536


class GuardedWorkspaces:
    def __init__(self, fill, slack=None):
        """fill: the byte every buffer is pre-filled with.  slack (nbytes -> extra bytes handed out behind the declaration;
        default none): the generous control run of the invariance checks"""
        assert 0 <= fill <= 0xFF
        self.fill = int(fill)
        self.slack = slack
        self.records = []                    # (tag, declared bytes, handed-out bytes, whole buffer)

    def __call__(self, nbytes, device, tag="ws"):
        nbytes = int(nbytes)
        assert nbytes >= 0, (tag, nbytes)
        handed = nbytes + (int(self.slack(nbytes)) if self.slack else 0)
        buf = torch.full((FRONT + 2 * handed + BACK,), self.fill, dtype=torch.uint8, device=device)
        view = buf[FRONT:FRONT + handed]
        assert view.numel() == handed and view.data_ptr() % 256 == 0, (tag, view.data_ptr())
        self.records.append((tag, nbytes, handed, buf))
        return view

    def last(self):
        """(view, whole buffer) of the latest request"""
        tag, nbytes, handed, buf = self.records[-1]
        return buf[FRONT:FRONT + handed], buf

    def untouched(self):
        """every byte of every buffer, handed-out part included, still holds the fill (a refused call launched nothing)"""
        return all(bool((buf == self.fill).all()) for _, _, _, buf in self.records)

    def check(self):
        """every byte in front of and behind each handed-out view still equals the fill"""
        torch.cuda.synchronize()
        for tag, nbytes, handed, buf in self.records:
            for name, lo, hi in (("front", 0, FRONT), ("back", FRONT + handed, buf.numel())):
                dirty = (buf[lo:hi] != self.fill).nonzero()
                if dirty.numel():
                    first, last = int(dirty[0]) + lo - FRONT, int(dirty[-1]) + lo - FRONT
                    raise AssertionError(
                        f"workspace '{tag}': {dirty.numel()} bytes of the {name} canary were written, offsets {first} .. {last} "
                        f"relative to the workspace; declared size {nbytes} bytes, handed out {handed}")
