"""The one implementation of "tap, collect, raise" for the launch tap (mpu_unet_set_launch_tap).

The tap is a C callback (ctypes CFUNCTYPE returning void): an exception raised inside it cannot cross the C frame -- ctypes prints
it and returns, pytest turns that into a PytestUnraisableExceptionWarning, and the test passes. So CHECKS INSIDE A TAP NEVER ASSERT
DIRECTLY: they run inside `tapped`, which catches whatever a check raises, keeps it, and raises ONE AssertionError after the body.

    with tapped(model, check, schedule_log=True) as tap:
        model.forward_backward(x, y, sw)
    lines = tap.log.splitlines()

  * per launch: synchronize, then check(li) inside try / except BaseException; repr + a short traceback are recorded
    (tap.failures), the launch is counted (tap.launches) and the pass goes on -- later launches are still checked;
  * the tap is removed (and the schedule log switched off) in `finally`, whatever the body or a check did;
  * after the body: AssertionError("<n> of <launches> tapped launches failed their check; the first: ...") with the first failure
    in full. An exception of the body itself is not replaced; the failures so far are attached to it as a note.

`api` is the installer (tests/test_replay_bounds_host.py drives the helper through a C function pointer with a stub); the default
one talks to the library and is created on first use, so that importing this module loads nothing.
"""
import ctypes as C
import traceback


class _LibApi:
    """install / remove through the library; synchronize through torch."""

    def __init__(self):
        import torch
        from multiplanarunet_amd import _lib
        self._lib, self._torch = _lib, torch
        self.FN = _lib.LAUNCH_TAP_FN

    def set_tap(self, model, cb):
        self._lib.call("mpu_unet_set_launch_tap", model._h, C.cast(cb, C.c_void_p) if cb is not None else None, None)

    def synchronize(self):
        self._torch.cuda.synchronize()

    def log_enable(self, on):
        self._lib.load().mpu_schedule_log_enable(1 if on else 0)

    def log_read(self):
        lib = self._lib.load()
        n = lib.mpu_schedule_log_read(None, 0)
        buf = C.create_string_buffer(int(n) + 1)
        lib.mpu_schedule_log_read(buf, n + 1)
        return buf.value.decode()


class tapped:
    def __init__(self, model, check, schedule_log=False, api=None):
        self.model, self.check, self.schedule_log = model, check, schedule_log
        self.api = api if api is not None else _LibApi()
        self.failures, self.launches, self.log = [], 0, ""
        self._cb = None

    def _on_launch(self, _user, pinfo):                      # (runs under a C frame: nothing may leave it)
        try:
            self.launches += 1
            self.api.synchronize()
            self.check(pinfo.contents)
        except BaseException as e:
            self.failures.append("launch %d: %r\n%s" % (self.launches, e, traceback.format_exc(limit=4)))

    def __enter__(self):
        self._cb = self.api.FN(self._on_launch)              # (kept alive on self for as long as the tap is installed)
        self.api.set_tap(self.model, self._cb)
        try:
            if self.schedule_log:
                self.api.log_enable(True)
        except BaseException:
            self.api.set_tap(self.model, None)
            raise
        return self

    def __exit__(self, etype, evalue, tb):
        try:
            if self.schedule_log:
                try:
                    if etype is None:
                        self.api.synchronize()
                        self.log = self.api.log_read()
                finally:
                    self.api.log_enable(False)
        finally:
            self.api.set_tap(self.model, None)
            self._cb = None
        if etype is not None:
            if self.failures and hasattr(evalue, "add_note"):
                evalue.add_note("(%d tapped launches had failed their check before; the first:\n%s)" % (len(self.failures), self.failures[0]))
            return False
        if self.failures:
            raise AssertionError("%d of %d tapped launches failed their check; the first:\n%s"
                                 % (len(self.failures), self.launches, self.failures[0]))
        return False
