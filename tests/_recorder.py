"""The library stand-in that drives an engine on the CPU: every rart_* entry is answered and recorded instead of launched."""


class Recorder:
    """records (name, arguments) of every rart_* call in `calls`.  Every entry returns 0 (success) except: rart_*_workspace_bytes ->
    `workspace` bytes, rart_gemm256_supported -> `gemm256`, any other rart_*_supported -> supported(name, args) when that is set"""

    def __init__(self, workspace=4096):
        self.calls, self.gemm256, self.supported, self.workspace = [], 0, None, workspace

    @property
    def descs(self):
        """the descriptors of the GEMM launches, in order"""
        return [a[0]._obj for n, a in self.calls if n in ('rart_conv_igemm_bf16', 'rart_gemm_pair_bf16')]

    def __getattr__(self, name):
        if not name.startswith('rart_'):
            raise AttributeError(name)
        if name == 'rart_gemm256_supported':
            return lambda *a: self.gemm256
        if name.endswith('_supported') and self.supported is not None:
            return lambda *a: self.supported(name, a)

        def call(*args):
            self.calls.append((name, args))
            return self.workspace if name.endswith('_workspace_bytes') else 0
        return call
