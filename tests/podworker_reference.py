"""Which words a podworker run checks, stated in Python independently of
podworker.hip. The tests compare the binary's dumps with this; nothing here
is derived from the binary."""

STRIDE = 4099          # the sampled run checks every multiple of this ...
HEAD_WINDOW = 1 << 16  # ... below this index, and then the last element


def reference_sample_set(n, verify_all=False):
    """The element indices a run over n elements brings back, in order: every
    element with --verify-all, otherwise the sorted multiples of 4099 below
    min(n, 65536), then n-1 (again, where it is such a multiple itself)."""
    if verify_all:
        return list(range(n))
    return sorted(i for i in range(min(n, HEAD_WINDOW))
                  if i % STRIDE == 0) + [n - 1]
