from ._functions import (MatmulLtState, MatMul4Bit, MatMul8bit, MatMul8bitLt, bmm_cublas, matmul,  # noqa: F401
                         matmul_4bit, matmul_cublas, mm_cublas)
