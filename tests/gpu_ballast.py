"""Ballast for the GPU tests that call the library on a stream that is still busy."""

_ballast = {}


def keep_busy(torch, repeat=1):
    """a millisecond or two of work on torch's current stream (`repeat` times as much), so that what is queued behind it has not begun
    when the library is called.  ONE tensor serves every caller: streams that are kept busy at the same time race on its contents, which nobody reads"""
    if "t" not in _ballast:
        _ballast["t"] = torch.zeros(1 << 25, dtype=torch.int64, device="cuda")
    for _ in range(8 * repeat):
        _ballast["t"].add_(1)
