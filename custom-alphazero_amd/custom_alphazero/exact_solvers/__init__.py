"""The reference's exact_solvers package on the device solver (c4_exact_solver.py)."""
from custom_alphazero.exact_solvers.c4_exact_solver import (SolverBudgetError, evaluate_boards_with_solution,
                                                            exact_policy_and_value, exact_ranked_moves_and_value)

__all__ = ["SolverBudgetError", "evaluate_boards_with_solution", "exact_policy_and_value",
           "exact_ranked_moves_and_value"]
