from ._functions import (MatMul4Bit, ffn_4bit, lora_shrink, lora_shrink_ids, matmul_4bit, matmul_4bit_experts, matmul_4bit_gated, matmul_4bit_grouped, matmul_4bit_lora, matmul_4bit_lora_ids,
                         moe_ffn_4bit, moe_route, moe_route_grouped, moe_topk, moe_topk_grouped)

__all__ = ["MatMul4Bit", "matmul_4bit", "matmul_4bit_experts", "matmul_4bit_grouped", "moe_ffn_4bit", "matmul_4bit_gated", "ffn_4bit", "matmul_4bit_lora", "lora_shrink", "lora_shrink_ids", "matmul_4bit_lora_ids", "moe_topk", "moe_route", "moe_topk_grouped", "moe_route_grouped"]
