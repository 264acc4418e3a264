"""Orders what a GPU test prepares with torch in front of the library call that follows.

The context's streams are non-blocking: they do not wait for the null stream, which is where torch.full, fill_, slice assignments
and arithmetic on device tensors run.  A library call issued right behind such a kernel (stream=None is the context's own stream)
can overtake it - a sentinel fill that lands after the call's stores puts the sentinel back over a result, an input still being
written is read half done.  include/brisk_hip.h tells a caller how the streams are ordered; the tests synchronise."""


def settled(*tensors):
    """the device idle - every fill and copy queued so far has landed -, then the arguments as they came (one tensor: itself)"""
    import torch
    torch.cuda.synchronize()
    return tensors[0] if len(tensors) == 1 else tensors
